// blokus_mcts_agent.hip -- the tree search of crl_blokus_mcts as a seated agent (crl_blokus_sample_mcts,
// crl_blokus_rollout_mcts, crl_blokus_step_single_mcts; the contract is in include/colosseum_hip.h), gfx950, wave64.
// The rules, the tables and the per-wave working set are blokus.hip's, taken in by including that file up to its kernels;
// the search is a COPY of blokus_mcts_kernel's text without the candidate root (blokus_mcts.hip: change them together),
// in a translation unit of its own so that blokus.hip's kernels and both blokus_mcts_kernel instances stay what they are.
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

namespace {

// ---- crl_blokus_mcts's tree: a copy of blokus_mcts.hip's constants and arithmetic (change them together)
constexpr int BLK_MCTS_NODE_BYTES = 24;
constexpr int BLK_MCTS_PATH = 340;
constexpr int BLK_MCTS_FIXED_BYTES = 1280;
constexpr int BLK_MCTS_TREE_LDS = 45056;
constexpr int BLK_MCTS_MAX_DEPTH = 336;
constexpr int BLK_MCTS_MAX_S = (BLK_MCTS_TREE_LDS - BLK_MCTS_FIXED_BYTES) / BLK_MCTS_NODE_BYTES - 1;
constexpr int BLK_MCTS_GROUP_R = 4;
constexpr uint32_t BLK_MCTS_UNKNOWN = 0xffffffffu;
// the fixed part: path (680) + playout counts (16) + 4 x 64 child slots (512) = 1,208 bytes, and the word that hands
// `best` to the other waves of a workgroup
constexpr int BLK_AGENT_BEST_OFFSET = BLK_MCTS_PATH * 2 + 16 + 4 * 64 * 2;
static_assert(BLK_AGENT_BEST_OFFSET == 1208 && BLK_AGENT_BEST_OFFSET % 4 == 0, "the fixed part crl_blokus_mcts uses");
static_assert(BLK_AGENT_BEST_OFFSET + 4 <= BLK_MCTS_FIXED_BYTES, "fixed part of a tree: no room for the best word");
static_assert(BLK_MCTS_MAX_S == 1823, "S_max is crl_blokus_mcts_max_simulations'");
static_assert(sizeof(BlkTables) + 4 * sizeof(WaveLds) + BLK_MCTS_TREE_LDS <= 65536, "a workgroup's 64 KB of LDS");

__device__ __forceinline__ uint32_t blk_wave_max(uint32_t v)
{
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false));   // row_shr:1
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false));   // row_shr:2
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false));   // row_shr:4
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false));   // row_shr:8
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));   // row_bcast:15 -> rows 1, 3
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));   // row_bcast:31 -> rows 2, 3
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

__device__ __forceinline__ uint64_t blk_mcts_div(const uint64_t num, const uint32_t den)
{
    uint64_t q = (uint64_t)((double)num / (double)den);
    const int64_t r = (int64_t)(num - q * (uint64_t)den);
    q = r < 0 ? q - 1u : (r >= (int64_t)den ? q + 1u : q);
    return q;
}

__device__ __forceinline__ uint64_t blk_mcts_isqrt(const uint64_t x)
{
    uint64_t s = (uint64_t)sqrt((double)x);
    s = s * s > x ? s - 1u : ((s + 1u) * (s + 1u) <= x ? s + 1u : s);
    return s;
}

__device__ __forceinline__ uint32_t blk_mcts_lg(const uint32_t n)
{
    const uint32_t m = 31u - (uint32_t)__clz((int)n);
    return 256u * m + (((n << (31u - m)) >> 23) & 255u);
}

// a tree's arrays in LDS (blokus_mcts_kernel's layout) and the best word behind them
struct BlkTree {
    uint32_t *n, *w;
    int32_t *id;
    uint32_t *rank, *l, *meta;
    uint16_t *path;
    uint32_t *cnt;
    uint16_t *kids;
    uint32_t *best;
};

// what a search is asked with: crl_blokus_mcts's W, S, R, cexp and the draws' key
struct BlkSearchArgs { int W, S, R; uint32_t cexp, seed_lo, seed_hi; };

// crl_blokus_mcts(cand = NULL, A = 1) on the position (root_a, root_b, root_vinv, root_vscore, round0, pl0) with the step
// counter tc0: `best`, in every wave of the tree.  blokus_mcts_kernel's text from the root's set-up to the pick of the most
// visited child, without the candidate root and the per-slot outputs (a copy: change them together).  It leaves the wave's
// board and rows in whatever state the last simulation left them.
template <bool GROUP>
__device__ __forceinline__ int blk_agent_search(const BlkTables &T, WaveLds &L, const int lane, const int wave_, const BlkTree &tr,
                                                const uint32_t root_a, const uint32_t root_b, const uint32_t root_vinv,
                                                const int root_vscore, const int round0, const int pl0, const uint32_t tc0,
                                                const uint32_t g, const BlkSearchArgs &sa, const uint32_t piece_cells,
                                                const BlkOwners &owners)
{
    const int W = sa.W, S = sa.S, R = sa.R;
    const uint32_t cexp = sa.cexp, seed_lo = sa.seed_lo, seed_hi = sa.seed_hi;
    const bool writer = !GROUP || wave_ == 0;
    auto tree_sync = [&]() {
        if (GROUP) __syncthreads();
        else wave_sync();
    };
    uint32_t *n_arr = tr.n, *w_arr = tr.w, *rank_arr = tr.rank, *l_arr = tr.l, *meta_arr = tr.meta, *cnt_sh = tr.cnt;
    int32_t *id_arr = tr.id;
    uint16_t *path = tr.path, *kids = tr.kids;
    uint32_t *flat = &L.occ[0][0];
    auto put_board = [&](const uint32_t a, const uint32_t bb) {
        flat[lane] = a;
        if (lane < 4 * BN - 64) flat[64 + lane] = bb;
        wave_sync();
    };
    auto gather = [&](const int v, const int nn) {
        for (int u = 1 + lane; u < nn; u += 64) {
            const uint32_t m = meta_arr[u];
            if ((int)(m & 0xffffu) == v) kids[(m >> 16) & 63u] = (uint16_t)u;
        }
        wave_sync();
    };
    if (writer && lane == 0) {
        n_arr[0] = 0u; w_arr[0] = 0u; id_arr[0] = -2; rank_arr[0] = 0u; l_arr[0] = BLK_MCTS_UNKNOWN; meta_arr[0] = 0u;
        path[0] = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) cnt_sh[c] = 0u;
    }
    tree_sync();
    int nn = 1;                                                  // nodes so far (every wave keeps its own count)
    for (int s = 0; s < S; ++s) {
        put_board(root_a, root_b);
        uint32_t vinv = root_vinv;
        int vscore = root_vscore;
        int round = round0, pl = pl0, v = 0, d = 0, term = 0;
        int new_slot = -1, new_id = -2, leaf = 0;
        uint32_t new_rank = 0u, new_l = BLK_MCTS_UNKNOWN;
        for (;;) {
            CRL_BOUNDS_LT(v, S + 1, 360);
            const uint32_t meta_v = (uint32_t)__builtin_amdgcn_readfirstlane((int)meta_arr[v]);
            const uint32_t n_v = (uint32_t)__builtin_amdgcn_readfirstlane((int)n_arr[v]);
            const int c = (int)(meta_v >> 24);
            bool expand = c < W && (uint32_t)(c * c) <= n_v;
            if (expand && c > 0) {                               // (with children the node's legal actions have been counted)
                const uint32_t lk = (uint32_t)__builtin_amdgcn_readfirstlane((int)l_arr[v]);
                expand = (uint32_t)c < max(lk, 1u);
            }
            if (expand) {
                blk_prep(L, lane, round);                        // every player's rows of the PRE-move board (:424)
                const uint32_t ip = (uint32_t)__builtin_amdgcn_readlane((int)vinv, pl);
                BlkMove mv = {0, 0, 0, 0, 0};
                new_l = blk_count(T, L, pl, ip, lane);
                new_slot = c;
                new_id = -1;                                     // the pass, when there is nothing to play
                if (new_l > 0u) {
                    const philox_out dr = philox4x32_10(g, 0x80000000u | (uint32_t)d, (uint32_t)s, CRL_TAG_BLOKUS_PLAYOUT, seed_lo, seed_hi);
                    uint32_t rho = __umulhi((uint32_t)__builtin_amdgcn_readfirstlane((int)dr.w[0]), new_l);
                    if (c > 0) gather(v, nn);
                    CRL_BOUNDS_LT(lane < c ? (int)kids[lane] : 0, S + 1, 361);
                    const uint32_t my_rank = lane < c ? rank_arr[kids[lane]] : BLK_MCTS_UNKNOWN;
                    while (__ballot(my_rank == rho) != 0ull) rho = rho + 1u == new_l ? 0u : rho + 1u;   // (c < L: it ends)
                    new_rank = rho;
                    mv = blk_select(T, L, pl, ip, rho, lane);
                    new_id = blk_encode(mv);
                }
                uint32_t inv[4];
                int score[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    inv[q] = (uint32_t)__builtin_amdgcn_readlane((int)vinv, q);
                    score[q] = __builtin_amdgcn_readlane(vscore, q);
                }
                if (new_id >= 0) (void)blk_apply(T, L, pl, mv, inv, score, lane);   // blk_play of a legal dense id: it returns 0
                term = blk_anyone_moves(T, L, inv, lane, &owners) ? 0 : 1;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    vinv = (lane & 3) == q ? inv[q] : vinv;
                    vscore = (lane & 3) == q ? score[q] : vscore;
                }
                round = blk_next_round(round, pl);
                pl = blk_next_mover(pl);
                d += 1;
                leaf = nn++;
                break;
            }
            // ---- select: lane k scores the child in slot k
            const unsigned long long have = c >= 64 ? ~0ull : (1ull << c) - 1ull;
            gather(v, nn);
            const bool mine = (have >> lane) & 1ull;
            const uint32_t cu = mine ? (uint32_t)kids[lane] : 0u;
            CRL_BOUNDS_LT(cu, S + 1, 362);
            uint32_t key = 0u;
            if (mine) {
                const uint32_t nu = n_arr[cu], wu = w_arr[cu];
                const uint64_t exploit = blk_mcts_div((uint64_t)wu << 16, nu * (uint32_t)R);
                const uint64_t X = blk_mcts_div((uint64_t)blk_mcts_lg(n_v) << 24, nu);
                key = (uint32_t)(exploit + (((uint64_t)cexp * blk_mcts_isqrt(X)) >> 8)) + 1u;   // < 2^27
            }
            const uint32_t top = blk_wave_max(key);              // (all lanes: outside the branch above)
            const int e = (int)__builtin_ctzll(__ballot(mine && key == top) | (1ull << 63));    // ties: the lowest slot
            const int u = __builtin_amdgcn_readlane((int)cu, e);
            const int id = __builtin_amdgcn_readfirstlane(id_arr[u]);
            term = (int)((((uint32_t)__builtin_amdgcn_readfirstlane((int)meta_arr[u])) >> 23) & 1u);
            if (id >= 0) {                                       // the child's ply: legal here, as when the child was made
                const BlkMove mv = blk_decode(id);
                const int n = __builtin_amdgcn_readlane((int)piece_cells, mv.piece);
                blk_place_legal(T, L, pl, mv, lane, n);
                const uint32_t left = vinv & ~(1u << mv.piece);  // ai.py:44-54 for the mover's lane(s)
                const bool me = (lane & 3) == pl;
                vscore += me ? n + (left == 0u ? (mv.piece == 0 ? 20 : 15) : 0) : 0;
                vinv = me ? left : vinv;
            }
            round = blk_next_round(round, pl);
            pl = blk_next_mover(pl);
            d += 1;
            CRL_BOUNDS_LT(d, BLK_MCTS_PATH, 363);
            if (writer && lane == 0) path[d] = (uint16_t)u;
            leaf = u;
            if (term || d >= BLK_MCTS_MAX_DEPTH) break;          // (d >= 336: never, see the contract)
            v = u;
        }
        tree_sync();                                             // ---- nobody reads the tree any more: the new node
        if (writer && new_slot >= 0 && lane == 0) {
            CRL_BOUNDS_LT(leaf, S + 1, 364);
            CRL_BOUNDS_LT(d, BLK_MCTS_PATH, 365);
            n_arr[leaf] = 0u; w_arr[leaf] = 0u; id_arr[leaf] = new_id; rank_arr[leaf] = new_rank; l_arr[leaf] = BLK_MCTS_UNKNOWN;
            meta_arr[leaf] = (uint32_t)v | (uint32_t)new_slot << 16 | (uint32_t)term << 23;
            meta_arr[v] += 1u << 24;
            if (new_l != BLK_MCTS_UNKNOWN) l_arr[v] = new_l;
            path[d] = (uint16_t)leaf;
        }
        // ---- evaluate the leaf: the winners of the ply into it, or R random playouts
        uint32_t cnt[4] = {0u, 0u, 0u, 0u};
        if (term) {
            const int score[4] = {__builtin_amdgcn_readlane(vscore, 0), __builtin_amdgcn_readlane(vscore, 1),
                                  __builtin_amdgcn_readlane(vscore, 2), __builtin_amdgcn_readlane(vscore, 3)};
            const uint32_t mask = (uint32_t)blk_outcome(false, 0, score).winners;
#pragma unroll
            for (int q = 0; q < 4; ++q) cnt[q] = ((mask >> q) & 1u) ? (uint32_t)R : 0u;
        } else {
            const uint32_t leaf_a = flat[lane], leaf_b = lane < 4 * BN - 64 ? flat[64 + lane] : 0u;
            const uint32_t leaf_vinv = vinv;
            const int leaf_vscore = vscore, leaf_round = round, leaf_pl = pl;
            for (int r = GROUP ? wave_ : 0; r < R; r += GROUP ? 4 : 1) {
                put_board(leaf_a, leaf_b);
                vinv = leaf_vinv; vscore = leaf_vscore; round = leaf_round; pl = leaf_pl;
                const uint32_t c2 = ((uint32_t)s << 16) | (uint32_t)r;
                uint32_t tc = tc0 + (uint32_t)d;
                uint32_t dead = 0, can_move = 0, rnd_word = 0u, winners_mask = 0u;
                bool over = false;
                // ---- random plies: blokus_playout_kernel's loop body under the search's counter words (a copy, as in
                // blokus_mcts_kernel)
                for (int t = 0; !over; ++t) {
                    const uint32_t ip = (uint32_t)__builtin_amdgcn_readlane((int)vinv, pl);
                    const BlkPrologue pro = blk_prologue(L, lane, round, pl, ip, owners);
                    uint32_t piece_incl = 0u, piece_cnt = 0u, total = 0u;
                    if (!((dead >> pl) & 1u) && pro.anchor_rows != 0u) {
                        const int lo = __builtin_ctz(pro.anchor_rows), hi = 31 - __builtin_clz(pro.anchor_rows);
                        total = blk_count_batches(T, L, lane, pro.items, lo, hi, &piece_incl, &piece_cnt);
                    }
                    if (total == 0 && round >= 1) dead |= 1u << pl;
                    if ((tc & 15u) == 0u || t == 0) {            // lane j < 16: the word of step counter (tc & ~15) + j
                        uint32_t k0 = seed_lo, k1 = seed_hi;
                        asm volatile("" : "+s"(k0), "+s"(k1));
                        const philox_out r4 = philox4x32_10(g, (((tc >> 4) << 2) + (uint32_t)((lane >> 2) & 3)) | 0x40000000u, c2,
                                                            CRL_TAG_BLOKUS_PLAYOUT, k0, k1);
                        const int ws = lane & 3;
                        rnd_word = ws == 0 ? r4.w[0] : ws == 1 ? r4.w[1] : ws == 2 ? r4.w[2] : r4.w[3];
                    }
                    const uint32_t word = (uint32_t)__builtin_amdgcn_readlane((int)rnd_word, (int)(tc & 15u));
                    tc += 1;
                    bool any_move = false;
                    BlkMove mv = {0, 0, 0, 0, 0};
                    if (total > 0) {
                        mv = blk_select<true>(T, L, pl, ip, __umulhi(word, total), lane, piece_incl, piece_cnt, piece_cells);
                        any_move = total > (uint32_t)__builtin_amdgcn_readlane((int)piece_cnt, mv.piece);
                    }
                    if (!any_move && (can_move & ~(1u << pl))) any_move = true;
                    for (int q = 0; q < 4 && !any_move; ++q) {   // the others, on the PRE-move board (:424)
                        if (q == pl || ((dead >> q) & 1u)) continue;
                        blk_prep(L, lane, round, q);
                        const uint32_t iq = (uint32_t)__builtin_amdgcn_readlane((int)vinv, q);
                        any_move = blk_exists(T, L, q, iq, lane, &owners);
                        if (any_move) can_move |= 1u << q;
                        if (!any_move && round >= 1) dead |= 1u << q;
                    }
                    if (total > 0) {
                        const int n = __builtin_amdgcn_readlane((int)piece_cells, mv.piece);
                        blk_place_legal(T, L, pl, mv, lane, n);
                        const uint32_t left = vinv & ~(1u << mv.piece);  // ai.py:44-54 for the mover's lane(s)
                        const bool me = (lane & 3) == pl;
                        vscore += me ? n + (left == 0u ? (mv.piece == 0 ? 20 : 15) : 0) : 0;
                        vinv = me ? left : vinv;
                        can_move = 0;
                    }
                    if (pl == 3) can_move = 0;
                    round += (pl == 3) ? 1 : 0;
                    pl = (pl + 1) & 3;
                    if (!any_move) {                             // terminal (BlokusEnvironment.py:424-440)
                        const int score[4] = {__builtin_amdgcn_readlane(vscore, 0), __builtin_amdgcn_readlane(vscore, 1),
                                              __builtin_amdgcn_readlane(vscore, 2), __builtin_amdgcn_readlane(vscore, 3)};
                        winners_mask = (uint32_t)blk_outcome(false, 0, score).winners;
                        over = true;
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) cnt[q] += (winners_mask >> q) & 1u;
            }
            if (GROUP) {                                         // the four waves' counts meet in LDS
                if (lane < 4) {
                    uint32_t mine = 0u;
#pragma unroll
                    for (int q = 0; q < 4; ++q) mine = (lane == q) ? cnt[q] : mine;
                    if (mine) atomicAdd(&cnt_sh[lane], mine);
                }
                __syncthreads();
            }
        }
        // ---- back up: lane i adds to the node at depth i (distinct nodes: no atomics), q = who moved into it
        if (writer) {
            wave_sync();                                         // (lane 0's path and node stores)
            if (GROUP && !term) {
#pragma unroll
                for (int q = 0; q < 4; ++q) cnt[q] = cnt_sh[q];
                wave_sync();
                if (lane < 4) cnt_sh[lane] = 0u;
            }
            for (int i = lane; i <= d; i += 64) {
                const uint32_t node = path[i];
                CRL_BOUNDS_LT(node, S + 1, 366);
                n_arr[node] += 1u;
                if (i > 0) {
                    const int q = (pl0 + i - 1) & 3;
                    uint32_t add = 0u;
#pragma unroll
                    for (int p = 0; p < 4; ++p) add = (p == q) ? cnt[p] : add;
                    w_arr[node] += add;
                }
            }
        }
        tree_sync();
    }
    // ---- the most visited child of the root (then the larger w, then the lowest slot)
    int best_id = -2;
    if (writer) {
        const uint32_t meta0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)meta_arr[0]);
        const int c0 = (int)(meta0 >> 24);
        const unsigned long long have = c0 >= 64 ? ~0ull : (1ull << c0) - 1ull;
        gather(0, nn);
        const bool mine = (have >> lane) & 1ull;
        const uint32_t cu = mine ? (uint32_t)kids[lane] : 0u;
        CRL_BOUNDS_LT(cu, S + 1, 367);
        const uint32_t vis = mine ? n_arr[cu] : 0u, val = mine ? w_arr[cu] : 0u;
        const int cid = mine ? id_arr[cu] : -2;
        const uint32_t top_n = blk_wave_max(vis);                // (a child has n >= 1)
        const bool most = mine && vis == top_n;
        const uint32_t top_w = blk_wave_max(most ? val + 1u : 0u);
        const unsigned long long pick = __ballot(most && val + 1u == top_w);
        best_id = pick ? __builtin_amdgcn_readlane(cid, (int)__builtin_ctzll(pick)) : -2;
        if (GROUP && lane == 0) *tr.best = (uint32_t)best_id;
    }
    if (GROUP) {                                                 // wave 0 hands `best` to the others
        __syncthreads();
        best_id = __builtin_amdgcn_readfirstlane((int)*tr.best);
    }
    return best_id;
}

// blk_write_observation of blokus.hip, which lies behind the point up to which this file includes it (a COPY: change them
// together)
// state_to_observation of game b for observer pl (BlokusEnvironment.py:752-768) by the wave that holds the game's row
// bitboards in LDS: board = -1 empty else (owner - observer) % 4, rotated by np.rot90(k=-pl), four cells (one dword) per
// lane and trip; pieces[r][i] = inventory bit i of player (r + observer) % 4; score rolled by -observer.
__device__ __forceinline__ void blk_agent_write_observation(const uint32_t (&occ)[4][BN], const uint32_t (&inv)[4], const int (&score)[4],
                                                      const int pl, const int64_t b, const int lane, int8_t *__restrict__ obs_board,
                                                      uint8_t *__restrict__ obs_pieces, int32_t *__restrict__ obs_score)
{
    for (int d = lane; d < BN * BN / 4; d += 64) {
        const int i = d / (BN / 4), j0 = (d - i * (BN / 4)) * 4;
        uint32_t word = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = j0 + k;
            int y, x;                                            // source cell of np.rot90(m, k=-pl)[i][j]
            switch (pl) {
                case 0: y = i; x = j; break;
                case 1: y = BN - 1 - j; x = i; break;
                case 2: y = BN - 1 - i; x = BN - 1 - j; break;
                default: y = j; x = BN - 1 - i; break;
            }
            int v = -1;
#pragma unroll
            for (int c = 0; c < 4; ++c) v = ((occ[c][y] >> x) & 1u) ? ((c - pl) & 3) : v;
            word |= (uint32_t)(v & 0xff) << (8 * k);
        }
        reinterpret_cast<uint32_t *>(obs_board + b * (BN * BN))[d] = word;
    }
    for (int cell = lane; cell < 4 * NPIECE; cell += 64) {       // pieces[r][piece] of player (r + observer) % 4
        const int r = cell / NPIECE, piece = cell - r * NPIECE;
        uint32_t iv = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) iv = (c == ((r + pl) & 3)) ? inv[c] : iv;
        obs_pieces[b * 4 * NPIECE + cell] = (uint8_t)((iv >> piece) & 1u);
    }
    if (lane < 4) {                                              // np.roll(score, -observer)
        int sc = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) sc = (c == ((lane + pl) & 3)) ? score[c] : sc;
        obs_score[b * 4 + lane] = sc;
    }
}

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
    BlkTree tr;
    tr.n = blk_agent_lds + (GROUP ? 0u : (uint32_t)wave_ * tree_words);
    tr.w = tr.n + (S + 1);
    tr.id = reinterpret_cast<int32_t *>(tr.w + (S + 1));
    tr.rank = tr.w + 2 * (S + 1);
    tr.l = tr.w + 3 * (S + 1);
    tr.meta = tr.w + 4 * (S + 1);
    tr.path = reinterpret_cast<uint16_t *>(tr.meta + (S + 1));
    tr.cnt = reinterpret_cast<uint32_t *>(tr.path + BLK_MCTS_PATH);
    tr.kids = reinterpret_cast<uint16_t *>(tr.cnt + 4) + (GROUP ? wave_ : 0) * 64;
    tr.best = reinterpret_cast<uint32_t *>(reinterpret_cast<uint16_t *>(tr.cnt + 4) + 4 * 64);
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
        const int id = blk_agent_search<GROUP>(T, L, lane, wave_, tr, pos_a, pos_b, vinv, vscore, round, pl, tc, g, sa, piece_cells, owners);
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
    blk_agent_write_observation(L.occ, inv, score, seat, b, lane, io.obs_board, io.obs_pieces, io.obs_score);
}

// the checks the three entries share, in the contract's order (the context's comes behind them, in the launcher)
#define BLK_AGENT_SEARCH_CHECK(fn)                                                                                      \
    CRL_REQUIRE(B > 0 && B <= ((int64_t)1 << 28), fn ": B=%lld out of range", (long long)B);                            \
    CRL_REQUIRE(W >= 1 && W <= 64, fn ": W=%d out of range 1..64", W);                                                  \
    CRL_REQUIRE(S >= 1 && S <= BLK_MCTS_MAX_S, fn ": S=%d out of range 1..%d", S, BLK_MCTS_MAX_S);                      \
    CRL_REQUIRE(R >= 1 && R <= 1024, fn ": R=%d out of range 1..1024", R);                                              \
    CRL_REQUIRE(cexp <= 65535u, fn ": cexp=%u out of range 0..65535", cexp);                                            \
    CRL_REQUIRE(noise >= 0.0 && noise <= 1.0, fn ": noise=%g outside [0, 1]", noise);   /* (NaN fails too) */           \
    CRL_REQUIRE(ctx != nullptr && ctx->game == CRL_GAME_BLOKUS && ctx->blokus, fn ": ctx is not a blokus context")

template <int FRAME>
int blk_agent_launch(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, uint32_t *occ, uint32_t *inv,
                     int32_t *score, int32_t *round, int32_t *to_move, int W, int S, int R, uint32_t cexp, double noise,
                     const BlkAgentIo &io, void *stream)
{
    const uint32_t tree_bytes = (uint32_t)(S + 1) * BLK_MCTS_NODE_BYTES + BLK_MCTS_FIXED_BYTES;
    const uint64_t thr = crl_noise_threshold(noise);
    if (R >= BLK_MCTS_GROUP_R) {                                  // a workgroup per game
        hipLaunchKernelGGL((blokus_mcts_agent_kernel<FRAME, true>), dim3((unsigned)B), dim3(256), tree_bytes, (hipStream_t)stream,
                           (const BlkTables *)ctx->blokus, B, (uint32_t)seed, (uint32_t)(seed >> 32), first_env_id,
                           occ, inv, score, round, to_move, W, S, R, cexp, thr, tree_bytes / 4u, 1, io);
    } else {                                                      // a wave per game, as many trees as fit beside each other
        const int fit = (int)(BLK_MCTS_TREE_LDS / tree_bytes), trees = fit < 4 ? fit : 4;
        hipLaunchKernelGGL((blokus_mcts_agent_kernel<FRAME, false>), dim3((unsigned)((B + trees - 1) / trees)), dim3(256),
                           trees * tree_bytes, (hipStream_t)stream, (const BlkTables *)ctx->blokus, B, (uint32_t)seed,
                           (uint32_t)(seed >> 32), first_env_id, occ, inv, score, round, to_move, W, S, R, cexp, thr,
                           tree_bytes / 4u, trees, io);
    }
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
