// blokus_mcts_agent.hip -- the tree search of crl_blokus_mcts as a seated agent (crl_blokus_sample_mcts,
// crl_blokus_rollout_mcts, crl_blokus_step_single_mcts; the contract is in include/colosseum_hip.h), gfx950, wave64.
// The rules, the tables and the per-wave working set are blokus.hip's, taken in by including that file up to its kernels;
// the search is blk_mcts_search (blokus_mcts_search.hpp), the text crl_blokus_mcts runs, asked without a candidate root; a
// translation unit of its own so that blokus.hip's kernels stay what they are.
//
// One kernel text, the frame a template parameter: one agent ply (sample), T plies with every seat on the agent (rollout),
// or crl_blokus_step_single's loop with the agent as the opponents (single).  The wave's LDS board (WaveLds) is the
// search's scratch -- every simulation overwrites it --, so the frame keeps the game's position outside it: the 80 row
// words in two VGPRs (lane i holds words i and 64 + i), inventories and scores one player per lane (lane & 3).  Before a
// ply the frame puts the position on the board and builds the allowed / corner rows, counts the mover's actions, and
// either passes (no action), draws the random agent's action (a noisy ply) or searches; after a search it puts the
// position back and plays the chosen ply by blk_next_state's steps, as the step entries do, and reads the board back into
// the two registers.  Everything around the search is wave-uniform: mover, seat, counters, the noise test, the count.
// Two mappings, as crl_blokus_mcts: R < 4 a wave per game (up to four games per workgroup as the trees fit), R >= 4 a
// workgroup per game.  In a workgroup every wave carries the game on its own WaveLds and replays the whole frame -- it is
// a function of state and counters, so the waves agree without talking and reach the same barriers: a noisy ply or a pass
// skips the search in all four alike --, wave 0 writes the tree, hands `best` to the others through LDS behind a barrier
// and alone stores state and outputs.
#define BLK_DEVICE_ONLY
#include "blokus.hip"
#include "blokus_mcts_search.hpp"

namespace {

enum { BLK_FRAME_SAMPLE = 0, BLK_FRAME_ROLLOUT = 1, BLK_FRAME_SINGLE = 2 };

// what a frame reads and writes besides the state: crl_blokus_sample's, crl_blokus_rollout's, crl_blokus_step_single's
struct BlkAgentIo {
    uint32_t *tcount;                                            // (the rollout's is st.tcount)
    int advance;
    int32_t *action;
    int T_steps;
    crl_blokus_stats st;
    const int8_t *seat;
    const int64_t *learner_action;
    int8_t *reward;
    uint8_t *done, *winners;
    int32_t *n_valid;
    int8_t *obs_board;
    uint8_t *obs_pieces;
    int32_t *obs_score;
    uint32_t flags;
};

// 4 waves per SIMD: the trees' LDS admits no more workgroups per CU than that anyway (as blokus_mcts_kernel)
template <int FRAME, bool GROUP>
__global__ void __launch_bounds__(256, 4)
blokus_mcts_agent_kernel(const BlkTables *__restrict__ tables, const int64_t B, const uint32_t seed_lo, const uint32_t seed_hi,
                         const uint64_t first_env_id, uint32_t *__restrict__ occ, uint32_t *__restrict__ inv_g,
                         int32_t *__restrict__ score_g, int32_t *__restrict__ round_g, int32_t *__restrict__ to_move_g,
                         const int W, const int S, const int R, const uint32_t cexp, const uint64_t thr,
                         const uint32_t tree_words, const int trees, const BlkAgentIo io)
{
    BLK_WAVE_SETUP();
    extern __shared__ __attribute__((aligned(16))) uint32_t blk_agent_lds[];
    if (!GROUP && wave_ >= trees) return;                       // (behind the set-up's barrier, the only one of this mapping)
    const int64_t b = GROUP ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * trees + wave_;
    if (b >= B) return;                                          // (a whole workgroup when GROUP)
    const bool writer = !GROUP || wave_ == 0;
    const BlkTree tr = blk_tree_layout<GROUP>(blk_agent_lds, wave_, tree_words, S);
    const BlkSearchArgs sa = {W, S, R, cexp, seed_lo, seed_hi};
    uint32_t *flat = &L.occ[0][0];                               // the board's 80 row words: lane i holds words i and 64 + i
    auto put_board = [&](const uint32_t a, const uint32_t bb) {
        flat[lane] = a;
        if (lane < 4 * BN - 64) flat[64 + lane] = bb;
        wave_sync();
    };
    const uint32_t piece_cells = lane < 24 ? T.ncell[lane] : 0u;
    const BlkOwners owners = blk_shape_owners(T, lane);
    // ---- the game's position, outside the board the search scribbles on
    uint32_t pos_a = occ[b * 4 * BN + lane], pos_b = lane < 4 * BN - 64 ? occ[b * 4 * BN + 64 + lane] : 0u;
    uint32_t vinv = inv_g[b * 4 + (lane & 3)];
    int vscore = score_g[b * 4 + (lane & 3)];
    int round = __builtin_amdgcn_readfirstlane(round_g[b]), pl = __builtin_amdgcn_readfirstlane(to_move_g[b]) & 3;
    uint32_t tc = (uint32_t)__builtin_amdgcn_readfirstlane((int)io.tcount[b]);
    const uint32_t g = (uint32_t)(first_env_id + (uint64_t)b);
    int seat = 0;
    uint32_t ts = 0u;
    if (FRAME == BLK_FRAME_SINGLE) seat = __builtin_amdgcn_readfirstlane((int)io.seat[b]) & 3;
    if (FRAME == BLK_FRAME_ROLLOUT) ts = (uint32_t)__builtin_amdgcn_readfirstlane((int)io.st.tstep[b]);
    if (GROUP) __syncthreads();                                  // every wave holds the game before wave 0 may store anything

    // the agent's action for the mover at step counter tc.  In: the position on the board with blk_prep's rows of `round`;
    // out: the same (a search is followed by putting both back)
    auto agent_action = [&]() -> int {
        const uint32_t ip = (uint32_t)__builtin_amdgcn_readlane((int)vinv, pl);
        const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)blk_count(T, L, pl, ip, lane));
        if (n == 0u) return -1;                                  // the pass: nothing is drawn, nothing is searched
        const philox_out nz = philox4x32_10(g, 0xC0000000u | (tc >> 2), 0u, CRL_TAG_BLOKUS_PLAYOUT, seed_lo, seed_hi);
        const uint32_t sel = tc & 3u;
        const uint32_t u = (uint32_t)__builtin_amdgcn_readfirstlane((int)(sel == 0 ? nz.w[0] : sel == 1 ? nz.w[1] : sel == 2 ? nz.w[2] : nz.w[3]));
        if ((uint64_t)u < thr) {                                 // a noisy ply: the random agent's action, no search
            const BlkMove mv = blk_select(T, L, pl, ip, __umulhi(blk_agent_word(g, tc, seed_lo, seed_hi), n), lane);
            return __builtin_amdgcn_readfirstlane(blk_encode(mv));
        }
        int id = blk_mcts_search<GROUP>(T, L, lane, wave_, tr, pos_a, pos_b, vinv, vscore, round, pl, tc, g, sa, piece_cells, owners,
                                        false, -3, 0ull, [](int, uint32_t, uint32_t, int, int) {});
        if (GROUP) {                                             // wave 0 hands `best` to the others
            if (writer && lane == 0) *tr.best = (uint32_t)id;
            __syncthreads();
            id = __builtin_amdgcn_readfirstlane((int)*tr.best);
        }
        if (FRAME != BLK_FRAME_SAMPLE) {
            put_board(pos_a, pos_b);
            blk_prep(L, lane, round);
        }
        return id;
    };
    // next_state (blk_next_state's text with the decoding spelt out) for `id` on the board as agent_action leaves it; a ply
    // that raises leaves everything as it was.  An agent's id is dense (DENSE): blk_decode.  The learner's may be an extended
    // one: blk_decode_any's arithmetic in selects -- through that function's two assignments of a BlkMove the compiler keeps
    // the move in scratch memory (12 bytes in every kernel that calls blk_play), which this kernel is to do without.
    auto play = [&](const int id, const bool dense) -> BlkPly {
        uint32_t inv[4];
        int score[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            inv[q] = (uint32_t)__builtin_amdgcn_readlane((int)vinv, q);
            score[q] = __builtin_amdgcn_readlane(vscore, q);
        }
        int status = 0;
        if (id >= 0) {
            const bool ext = !dense && id >= ACTION_IDS;
            const int a = ext ? id - CRL_BLOKUS_EXT_BASE : id;
            const int cell_d = (a / 40) % 400, cell_e = (a / 40) % 1600;
            BlkMove mv;
            mv.shift = a % 5;
            mv.orient = (a / 5) & 7;
            mv.piece = ext ? a / 64000 : a / 16000;
            mv.x = ext ? cell_e % 40 - BN : cell_d % BN;
            mv.y = ext ? cell_e / 40 - BN : cell_d / BN;
            status = ext && a >= CRL_BLOKUS_EXT_IDS ? CRL_BLOKUS_BAD_ACTION : blk_apply(T, L, pl, mv, inv, score, lane);
        }
        BlkPly ply = {status, status, 0, 0, round, pl};
        if (status == 0) {
            const BlkOutcome out = blk_outcome(blk_anyone_moves(T, L, inv, lane), pl, score);
            ply = BlkPly{0, out.reward, out.terminal, out.winners, blk_next_round(round, pl), blk_next_mover(pl)};
        }
        if (ply.status == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                vinv = (lane & 3) == q ? inv[q] : vinv;
                vscore = (lane & 3) == q ? score[q] : vscore;
            }
            wave_sync();
            pos_a = flat[lane];
            pos_b = lane < 4 * BN - 64 ? flat[64 + lane] : 0u;
            round = ply.round;
            pl = ply.pl;
        }
        return ply;
    };
    auto fresh = [&]() {
        pos_a = 0u; pos_b = 0u;
        vinv = (1u << NPIECE) - 1u;
        vscore = 0;
        round = 0; pl = 0;
    };

    if (FRAME == BLK_FRAME_SAMPLE) {
        put_board(pos_a, pos_b);
        blk_prep(L, lane, round);
        const int id = agent_action();
        if (writer && lane == 0) {
            io.action[b] = id;
            if (io.advance) io.tcount[b] = tc + 1u;
        }
        return;
    }

    if (FRAME == BLK_FRAME_ROLLOUT) {
        for (int t = 0; t < io.T_steps; ++t) {
            put_board(pos_a, pos_b);
            blk_prep(L, lane, round);                            // allowed / corner rows of the PRE-move board (:424)
            const int id = agent_action();
            const BlkPly ply = play(id, true);                   // (an agent's action is legal: status 0)
            tc += 1u;
            ts += 1u;
            if (ply.terminal) {                                  // crl_blokus_rollout's bookkeeping and auto-reset
                if (writer && lane < 4) {
                    const int64_t c = lane;
                    io.st.win_count[c * B + b] += (uint32_t)((ply.winners >> lane) & 1);
                    io.st.score_sum[c * B + b] += vscore;
                }
                if (writer && lane == 0) {
                    io.st.n_episodes[b] += 1;
                    io.st.len_sum[b] += ts;
                }
                fresh();
                ts = 0u;
            }
        }
        if (!writer) return;
        occ[b * 4 * BN + lane] = pos_a;
        if (lane < 4 * BN - 64) occ[b * 4 * BN + 64 + lane] = pos_b;
        if (lane < 4) { inv_g[b * 4 + lane] = vinv; score_g[b * 4 + lane] = vscore; }
        if (lane == 0) {
            round_g[b] = round; to_move_g[b] = pl;
            io.st.tcount[b] = tc; io.st.tstep[b] = ts;
        }
        if (io.st.results && lane < 4) {                         // the packed row, from the running totals: every lane reads
            int32_t *row = io.st.results + b * 10;               // back what it wrote itself (program order: no fence needed)
            if (lane == 0) {
                row[0] = (int32_t)io.st.n_episodes[b];
                row[1] = (int32_t)io.st.len_sum[b];
            }
            row[2 + lane] = (int32_t)io.st.win_count[(int64_t)lane * B + b];
            row[6 + lane] = io.st.score_sum[(int64_t)lane * B + b];
        }
        return;
    }

    // ---- BLK_FRAME_SINGLE: blokus_step_single_kernel's loop (a copy: change them together) with the agent as the opponents
    int rew = 0, dn_wn = 0;                                      // dn_wn: done | winners << 1
    // plies: bit 3 = the next ply is the learner's, bits 0..2 = opponent plies played
    int plies = (io.learner_action != nullptr && pl == seat) ? 8 : 0;
    for (; plies >= 8 || (pl != seat && plies < 6); ) {
        const bool learner = plies >= 8;
        put_board(pos_a, pos_b);
        blk_prep(L, lane, round);                                // allowed / corner rows of the PRE-move board (:424)
        int id = -1;
        if (!learner) {
            id = agent_action();
        } else if (!(io.flags & CRL_STEP_RANK_ACTION)) {         // crl_blokus_step's int32 action; v < -1 is the pass
            const int64_t v = io.learner_action[b];
            const int64_t top = (int64_t)CRL_BLOKUS_EXT_BASE + CRL_BLOKUS_EXT_IDS;
            id = __builtin_amdgcn_readfirstlane(v < 0 ? -1 : (int)(v < top ? v : top));
        } else {                                                 // a rank into the learner's ordered legal list
            const uint32_t ip = (uint32_t)__builtin_amdgcn_readlane((int)vinv, pl);
            const uint32_t total = blk_count(T, L, pl, ip, lane);
            const int64_t r = io.learner_action[b];
            const int ri = __builtin_amdgcn_readfirstlane(r >= 0 && r < (int64_t)total ? (int)r : -1);
            if (ri >= 0) {
                const BlkMove mv = blk_select(T, L, pl, ip, (uint32_t)ri, lane);
                id = blk_encode(mv);
            }
        }
        plies = learner ? 0 : plies + 1;
        const BlkPly ply = play(id, !learner);
        if (ply.status != 0) { rew = ply.status; break; }        // (the learner's ply only: an agent's action is legal)
        tc += 1u;
        if (ply.terminal) {                                      // the learner's rank (:424-440 with the mover = seat), restart
            const int score[4] = {__builtin_amdgcn_readlane(vscore, 0), __builtin_amdgcn_readlane(vscore, 1),
                                  __builtin_amdgcn_readlane(vscore, 2), __builtin_amdgcn_readlane(vscore, 3)};
            dn_wn = 1 | ply.winners << 1;
            rew = blk_outcome(false, seat, score).reward;
            fresh();
        }
    }
    if (!writer) return;
    occ[b * 4 * BN + lane] = pos_a;
    if (lane < 4 * BN - 64) occ[b * 4 * BN + 64 + lane] = pos_b;
    if (lane < 4) { inv_g[b * 4 + lane] = vinv; score_g[b * 4 + lane] = vscore; }
    if (lane == 0) {
        round_g[b] = round;
        to_move_g[b] = pl;
        io.tcount[b] = tc;
        io.reward[b] = (int8_t)rew;
        io.done[b] = (uint8_t)(dn_wn & 1);
        io.winners[b] = (uint8_t)(dn_wn >> 1);
    }
    // ---- what the learner needs: its number of legal actions and its observation (:453-500, :752-768)
    put_board(pos_a, pos_b);
    blk_prep(L, lane, round);
    uint32_t inv[4];
    int score[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        inv[q] = (uint32_t)__builtin_amdgcn_readlane((int)vinv, q);
        score[q] = __builtin_amdgcn_readlane(vscore, q);
    }
    const uint32_t total = blk_count(T, L, seat, blk_pick(inv, seat), lane);
    if (lane == 0) io.n_valid[b] = (int32_t)total;
    blk_write_observation(L.occ, inv, score, seat, b, lane, io.obs_board, io.obs_pieces, io.obs_score);
}

// the checks the three entries share, in the contract's order (the context's comes behind them, in the launcher)
#define BLK_AGENT_SEARCH_CHECK(fn)                                                                                      \
    BLK_MCTS_BATCH_CHECK(fn);                                                                                           \
    BLK_MCTS_SEARCH_CHECK(fn);                                                                                          \
    CRL_REQUIRE(noise >= 0.0 && noise <= 1.0, fn ": noise=%g outside [0, 1]", noise);   /* (NaN fails too) */           \
    CRL_REQUIRE(ctx != nullptr && ctx->game == CRL_GAME_BLOKUS && ctx->blokus, fn ": ctx is not a blokus context")

template <int FRAME>
int blk_agent_launch(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, uint32_t *occ, uint32_t *inv,
                     int32_t *score, int32_t *round, int32_t *to_move, int W, int S, int R, uint32_t cexp, double noise,
                     const BlkAgentIo &io, void *stream)
{
    const uint64_t thr = crl_noise_threshold(noise);
    blk_mcts_dispatch(B, S, R, [&](auto group, unsigned grid, uint32_t lds_bytes, uint32_t tree_words, int trees) {
        hipLaunchKernelGGL((blokus_mcts_agent_kernel<FRAME, decltype(group)::value>), dim3(grid), dim3(256), lds_bytes,
                           (hipStream_t)stream, (const BlkTables *)ctx->blokus, B, (uint32_t)seed, (uint32_t)(seed >> 32),
                           first_env_id, occ, inv, score, round, to_move, W, S, R, cexp, thr, tree_words, trees, io);
    });
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

} // namespace

int crl_blokus_mcts_agent_bounds(unsigned int *out4)
{
    CRL_BOUNDS_READBACK(out4);
    return CRL_OK;
}

extern "C" {

int crl_blokus_sample_mcts(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, const uint32_t *occ,
                           const uint32_t *inv, const int32_t *score, const int32_t *round, const int32_t *to_move,
                           uint32_t *tcount, int advance, int W, int S, int R, uint32_t cexp, double noise,
                           int32_t *action, void *stream)
{
    // (the pointer and argument checks come before the context's: they need no device)
    CRL_REQUIRE(occ && inv && score && round && to_move && tcount && action, "crl_blokus_sample_mcts: NULL pointer");
    BLK_AGENT_SEARCH_CHECK("crl_blokus_sample_mcts");
    BlkAgentIo io = {};
    io.tcount = tcount; io.advance = advance; io.action = action;
    return blk_agent_launch<BLK_FRAME_SAMPLE>(ctx, B, seed, first_env_id, const_cast<uint32_t *>(occ), const_cast<uint32_t *>(inv),
                                              const_cast<int32_t *>(score), const_cast<int32_t *>(round),
                                              const_cast<int32_t *>(to_move), W, S, R, cexp, noise, io, stream);
}

int crl_blokus_rollout_mcts(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, int T, int W, int S, int R,
                            uint32_t cexp, double noise, uint32_t *occ, uint32_t *inv, int32_t *score, int32_t *round,
                            int32_t *to_move, crl_blokus_stats st, void *stream)
{
    CRL_REQUIRE(occ && inv && score && round && to_move, "crl_blokus_rollout_mcts: NULL state pointer");
    CRL_REQUIRE(st.tcount && st.tstep && st.n_episodes && st.win_count && st.len_sum && st.score_sum,
                "crl_blokus_rollout_mcts: NULL stats pointer");
    CRL_REQUIRE(T >= 0 && T <= (1 << 24), "crl_blokus_rollout_mcts: T=%d out of range", T);
    BLK_AGENT_SEARCH_CHECK("crl_blokus_rollout_mcts");
    if (T == 0) return CRL_OK;
    BlkAgentIo io = {};
    io.tcount = st.tcount; io.T_steps = T; io.st = st;
    return blk_agent_launch<BLK_FRAME_ROLLOUT>(ctx, B, seed, first_env_id, occ, inv, score, round, to_move, W, S, R, cexp, noise, io,
                                               stream);
}

int crl_blokus_step_single_mcts(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id,
                                uint32_t *occ, uint32_t *inv, int32_t *score, int32_t *round, int32_t *to_move,
                                const int8_t *seat, const int64_t *learner_action, uint32_t *tcount,
                                int8_t *reward, uint8_t *done, uint8_t *winners, int32_t *n_valid,
                                int8_t *obs_board, uint8_t *obs_pieces, int32_t *obs_score,
                                int W, int S, int R, uint32_t cexp, double noise, uint32_t flags, void *stream)
{
    CRL_REQUIRE(occ && inv && score && round && to_move, "crl_blokus_step_single_mcts: NULL state pointer");
    CRL_REQUIRE(seat && tcount, "crl_blokus_step_single_mcts: NULL seat / tcount pointer");
    CRL_REQUIRE(reward && done && winners && n_valid && obs_board && obs_pieces && obs_score,
                "crl_blokus_step_single_mcts: NULL output pointer");
    CRL_REQUIRE((flags & ~CRL_STEP_RANK_ACTION) == 0, "crl_blokus_step_single_mcts: unknown flags 0x%x", flags);
    CRL_REQUIRE((((uintptr_t)obs_board) & 3) == 0, "crl_blokus_step_single_mcts: obs_board must be 4-byte aligned");
    BLK_AGENT_SEARCH_CHECK("crl_blokus_step_single_mcts");
    BlkAgentIo io = {};
    io.tcount = tcount; io.seat = seat; io.learner_action = learner_action; io.reward = reward; io.done = done;
    io.winners = winners; io.n_valid = n_valid; io.obs_board = obs_board; io.obs_pieces = obs_pieces; io.obs_score = obs_score;
    io.flags = flags;
    return blk_agent_launch<BLK_FRAME_SINGLE>(ctx, B, seed, first_env_id, occ, inv, score, round, to_move, W, S, R, cexp, noise, io,
                                              stream);
}

} // extern "C"
