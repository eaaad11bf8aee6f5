// blokus_mcts_search.hpp -- the Blokus tree search itself, stated once for crl_blokus_mcts (blokus_mcts.hip) and the seated
// search agent (blokus_mcts_agent.hip): the tree's constants and layout in LDS, the score arithmetic, the search from the
// root's set-up to the root row, and what the two launchers share on the host.  Both units include it behind
// `#define BLK_DEVICE_ONLY` / `#include "blokus.hip"`, whose rules, tables and per-wave working set it uses.
//
// One tree in LDS, built by one wave (GROUP = false: up to four trees per workgroup) or by the four waves of a workgroup
// (GROUP = true).  In a workgroup every wave replays the whole descent on its own WaveLds from the shared tree -- the
// descent is a function of the tree and the counters, so the waves agree without talking --, wave 0 alone writes the
// tree, and the R playouts of the leaf are shared out, playout r to wave r & 3.  Per simulation the waves meet three
// times: behind the descent (nobody reads the tree any more: the new node is made), behind the playouts (their counts
// are in LDS) and behind the backup.  With one wave per tree these are wave barriers.
// A tree is six dword arrays of S + 1 entries -- n, w, the dense id of the move into the node, that move's rank in its
// parent's legal list, the node's own count of legal actions (BLK_MCTS_UNKNOWN until an expansion there has counted
// them) and meta = parent | slot << 16 | terminal << 23 | children << 24 -- and a fixed part: the path (node per depth),
// the four playout counts of a workgroup, per wave the 64 child slots of the node being looked at, and the word through
// which the agent's wave 0 hands `best` to the others.  Children are not listed per node (64 slots would be 128 bytes of
// every node): the lanes scan the nodes made so far for those whose parent is v and drop them into the slot array, lane k
// then is child k -- the rank probe of an expansion is a ballot over the children's ranks, the selection a wave maximum
// over their scores.
// The descent through existing nodes costs blk_place_legal per ply; an expansion pays blk_prep, a count pass, blk_select
// and the terminal test (blk_anyone_moves on the pre-move rows, as blk_next_state).
// The leaf's playouts are blokus_playout_kernel's ply loop under the search's counter words -- a COPY, as that loop is
// one of blokus_rollout_kernel's (see the comment above blokus_playout_kernel): change the three together.
#pragma once

namespace {

constexpr int BLK_MCTS_NODE_BYTES = 24;
constexpr int BLK_MCTS_PATH = 340;                           // path entries: depth 0 .. 336, rounded up
constexpr int BLK_MCTS_FIXED_BYTES = 1280;                   // path (680) + counts (16) + 4 x 64 child slots (512) + best (4), rounded up
constexpr int BLK_MCTS_BEST_OFFSET = BLK_MCTS_PATH * 2 + 16 + 4 * 64 * 2;
constexpr int BLK_MCTS_TREE_LDS = 45056;                     // what a workgroup's trees may take beside T and Lw[4] (18,560 B)
constexpr int BLK_MCTS_MAX_DEPTH = 336;
constexpr int BLK_MCTS_MAX_S = (BLK_MCTS_TREE_LDS - BLK_MCTS_FIXED_BYTES) / BLK_MCTS_NODE_BYTES - 1;   // 1823 (< 2^16: s fits its counter bits)
constexpr int BLK_MCTS_GROUP_R = 4;                          // R >= this: one workgroup per tree
constexpr uint32_t BLK_MCTS_UNKNOWN = 0xffffffffu;
static_assert(BLK_MCTS_BEST_OFFSET == 1208 && BLK_MCTS_BEST_OFFSET % 4 == 0, "the fixed part of a tree");
static_assert(BLK_MCTS_BEST_OFFSET + 4 <= BLK_MCTS_FIXED_BYTES, "fixed part of a tree: no room for the best word");
static_assert(BLK_MCTS_MAX_S == 1823, "S_max is crl_blokus_mcts_max_simulations'");
static_assert(sizeof(BlkTables) + 4 * sizeof(WaveLds) + BLK_MCTS_TREE_LDS <= 65536, "a workgroup's 64 KB of LDS");

// the maximum of v over the 64 lanes, in every lane (wave_scan_incl's DPP steps with max; every lane must run it)
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

// floor(num / den) for num < 2^52 and 1 <= den < 2^32 (the double quotient is within one of it), the exact floor square
// root of x < 2^52, and the contract's piecewise-linear log2 with 8 fraction bits: crl_ttt_mcts's score arithmetic
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

// a tree's arrays in LDS and the best word behind them
struct BlkTree {
    uint32_t *n, *w;
    int32_t *id;
    uint32_t *rank, *l, *meta;
    uint16_t *path;
    uint32_t *cnt;
    uint16_t *kids;
    uint32_t *best;
};

// the tree of wave `wave_` in the workgroup's dynamic LDS: with GROUP the one tree all four waves share (each with child
// slots of its own), else one of up to four, tree_words dwords apart
template <bool GROUP>
__device__ __forceinline__ BlkTree blk_tree_layout(uint32_t *lds, const int wave_, const uint32_t tree_words, const int S)
{
    BlkTree tr;
    tr.n = lds + (GROUP ? 0u : (uint32_t)wave_ * tree_words);
    tr.w = tr.n + (S + 1);
    tr.id = reinterpret_cast<int32_t *>(tr.w + (S + 1));
    tr.rank = tr.w + 2 * (S + 1);
    tr.l = tr.w + 3 * (S + 1);
    tr.meta = tr.w + 4 * (S + 1);
    tr.path = reinterpret_cast<uint16_t *>(tr.meta + (S + 1));
    tr.cnt = reinterpret_cast<uint32_t *>(tr.path + BLK_MCTS_PATH);
    tr.kids = reinterpret_cast<uint16_t *>(tr.cnt + 4) + (GROUP ? wave_ : 0) * 64;
    tr.best = reinterpret_cast<uint32_t *>(reinterpret_cast<uint16_t *>(tr.cnt + 4) + 4 * 64);
    return tr;
}

// what a search is asked with: crl_blokus_mcts's W, S, R, cexp and the draws' key
struct BlkSearchArgs { int W, S, R; uint32_t cexp, seed_lo, seed_hi; };

// crl_blokus_mcts on the position (root_a, root_b, root_vinv, root_vscore, round0, pl0) with the step counter tc0, in every
// wave of the tree.  With has_cand the root's children are the candidates: lane a holds column a's id in cand_v, and
// `playable` has the bits of the columns to search (not zero); without (false, -3, 0 as constants fold those paths away)
// the root widens as every other node.  The tree's writer wave hands the root row to root_row(id, visits, value, nodes,
// best) -- lane k the child in slot k (-2, 0, 0 where there is none), `best` the most visited child (then the larger w,
// then the lowest slot) -- and returns `best`; the other waves of a workgroup return -2.  (The row goes through a callable,
// not back by value: returned, blokus_mcts_kernel computed the addresses of its five stores in vector registers, 17 to 20
// VALU instructions and one or two VGPRs more.)  It leaves the wave's board and rows as the last simulation left them.
template <bool GROUP, typename RootRow>
__device__ __forceinline__ int blk_mcts_search(const BlkTables &T, WaveLds &L, const int lane, const int wave_, const BlkTree &tr,
                                               const uint32_t root_a, const uint32_t root_b, const uint32_t root_vinv,
                                               const int root_vscore, const int round0, const int pl0, const uint32_t tc0,
                                               const uint32_t g, const BlkSearchArgs &sa, const uint32_t piece_cells,
                                               const BlkOwners &owners, const bool has_cand, const int cand_v,
                                               const unsigned long long playable, RootRow &&root_row)
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
    uint32_t *flat = &L.occ[0][0];                               // the board's 80 row words: lane i holds words i and 64 + i
    auto put_board = [&](const uint32_t a, const uint32_t bb) {
        flat[lane] = a;
        if (lane < 4 * BN - 64) flat[64 + lane] = bb;
        wave_sync();
    };
    // the children of node v (nn nodes so far) into kids[slot]
    auto gather = [&](const int v, const int nn) {
        for (int u = 1 + lane; u < nn; u += 64) {
            const uint32_t m = meta_arr[u];
            if ((int)(m & 0xffffu) == v) kids[(m >> 16) & 63u] = (uint16_t)u;
        }
        wave_sync();
    };
    unsigned long long root_have = 0ull;                         // a candidate root: the playable columns that are children
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
        // what an expansion leaves for the writer: the new node and its parent's count of legal actions
        int new_slot = -1, new_id = -2, leaf = 0;
        uint32_t new_rank = 0u, new_l = BLK_MCTS_UNKNOWN;
        for (;;) {
            CRL_BOUNDS_LT(v, S + 1, 350);
            const uint32_t meta_v = (uint32_t)__builtin_amdgcn_readfirstlane((int)meta_arr[v]);
            const uint32_t n_v = (uint32_t)__builtin_amdgcn_readfirstlane((int)n_arr[v]);
            const int c = (int)(meta_v >> 24);
            const bool cand_root = has_cand && v == 0;
            const unsigned long long fresh = playable & ~root_have;
            bool expand;
            if (cand_root) {
                expand = fresh != 0ull;
            } else {
                expand = c < W && (uint32_t)(c * c) <= n_v;
                if (expand && c > 0) {                           // (with children the node's legal actions have been counted)
                    const uint32_t lk = (uint32_t)__builtin_amdgcn_readfirstlane((int)l_arr[v]);
                    expand = (uint32_t)c < max(lk, 1u);
                }
            }
            if (expand) {
                blk_prep(L, lane, round);                        // every player's rows of the PRE-move board (:424)
                const uint32_t ip = (uint32_t)__builtin_amdgcn_readlane((int)vinv, pl);
                BlkMove mv = {0, 0, 0, 0, 0};
                if (cand_root) {
                    new_slot = (int)__builtin_ctzll(fresh);
                    new_id = __builtin_amdgcn_readlane(cand_v, new_slot);
                    mv = blk_decode(new_id);
                    root_have |= 1ull << new_slot;
                } else {
                    new_l = blk_count(T, L, pl, ip, lane);
                    new_slot = c;
                    new_id = -1;                                 // the pass, when there is nothing to play
                    if (new_l > 0u) {
                        const philox_out dr = philox4x32_10(g, 0x80000000u | (uint32_t)d, (uint32_t)s, CRL_TAG_BLOKUS_PLAYOUT, seed_lo, seed_hi);
                        uint32_t rho = __umulhi((uint32_t)__builtin_amdgcn_readfirstlane((int)dr.w[0]), new_l);
                        if (c > 0) gather(v, nn);
                        CRL_BOUNDS_LT(lane < c ? (int)kids[lane] : 0, S + 1, 351);
                        const uint32_t my_rank = lane < c ? rank_arr[kids[lane]] : BLK_MCTS_UNKNOWN;
                        while (__ballot(my_rank == rho) != 0ull) rho = rho + 1u == new_l ? 0u : rho + 1u;   // (c < L: it ends)
                        new_rank = rho;
                        mv = blk_select(T, L, pl, ip, rho, lane);
                        new_id = blk_encode(mv);
                    }
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
            const unsigned long long have = cand_root ? root_have : (c >= 64 ? ~0ull : (1ull << c) - 1ull);
            gather(v, nn);
            const bool mine = (have >> lane) & 1ull;
            const uint32_t cu = mine ? (uint32_t)kids[lane] : 0u;
            CRL_BOUNDS_LT(cu, S + 1, 352);
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
            CRL_BOUNDS_LT(d, BLK_MCTS_PATH, 353);
            if (writer && lane == 0) path[d] = (uint16_t)u;
            leaf = u;
            if (term || d >= BLK_MCTS_MAX_DEPTH) break;          // (d >= 336: never, see the contract)
            v = u;
        }
        tree_sync();                                             // ---- nobody reads the tree any more: the new node
        if (writer && new_slot >= 0 && lane == 0) {
            CRL_BOUNDS_LT(leaf, S + 1, 354);
            CRL_BOUNDS_LT(d, BLK_MCTS_PATH, 355);
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
                // ---- random plies: blokus_playout_kernel's loop body under the search's counter words (a copy, see above)
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
                CRL_BOUNDS_LT(node, S + 1, 356);
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
    // ---- the root's children: id, visits, value, the most visited (then the larger w, then the lowest slot)
    int best_id = -2;
    if (writer) {
        const uint32_t meta0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)meta_arr[0]);
        const int c0 = (int)(meta0 >> 24);
        const unsigned long long have = has_cand ? root_have : (c0 >= 64 ? ~0ull : (1ull << c0) - 1ull);
        gather(0, nn);
        const bool mine = (have >> lane) & 1ull;
        const uint32_t cu = mine ? (uint32_t)kids[lane] : 0u;
        CRL_BOUNDS_LT(cu, S + 1, 357);
        const uint32_t vis = mine ? n_arr[cu] : 0u, val = mine ? w_arr[cu] : 0u;
        const int cid = mine ? id_arr[cu] : -2;
        const uint32_t top_n = blk_wave_max(vis);                // (a child has n >= 1)
        const bool most = mine && vis == top_n;
        const uint32_t top_w = blk_wave_max(most ? val + 1u : 0u);
        const unsigned long long pick = __ballot(most && val + 1u == top_w);
        best_id = pick ? __builtin_amdgcn_readlane(cid, (int)__builtin_ctzll(pick)) : -2;
        root_row(cid, vis, val, nn, best_id);
    }
    return best_id;
}

// ---- the host side both launchers share

// the checks every search entry makes on B and on W, S, R and cexp, in the contract's order (two macros: crl_blokus_mcts
// checks A between them)
#define BLK_MCTS_BATCH_CHECK(fn) CRL_REQUIRE(B > 0 && B <= ((int64_t)1 << 28), fn ": B=%lld out of range", (long long)B)
#define BLK_MCTS_SEARCH_CHECK(fn)                                                                                       \
    CRL_REQUIRE(W >= 1 && W <= 64, fn ": W=%d out of range 1..64", W);                                                  \
    CRL_REQUIRE(S >= 1 && S <= BLK_MCTS_MAX_S, fn ": S=%d out of range 1..%d", S, BLK_MCTS_MAX_S);                      \
    CRL_REQUIRE(R >= 1 && R <= 1024, fn ": R=%d out of range 1..1024", R);                                              \
    CRL_REQUIRE(cexp <= 65535u, fn ": cexp=%u out of range 0..65535", cexp)

// the two mappings: launch(GROUP as a std::bool_constant, workgroups, dynamic LDS bytes, tree_words, trees) with a workgroup
// per tree for R >= BLK_MCTS_GROUP_R, else a wave per tree and as many trees per workgroup as fit beside each other
template <typename Launch>
void blk_mcts_dispatch(const int64_t B, const int S, const int R, Launch &&launch)
{
    const uint32_t tree_bytes = (uint32_t)(S + 1) * BLK_MCTS_NODE_BYTES + BLK_MCTS_FIXED_BYTES;
    if (R >= BLK_MCTS_GROUP_R) {
        launch(std::true_type{}, (unsigned)B, tree_bytes, tree_bytes / 4u, 1);
    } else {
        const int fit = (int)(BLK_MCTS_TREE_LDS / tree_bytes), trees = fit < 4 ? fit : 4;
        launch(std::false_type{}, (unsigned)((B + trees - 1) / trees), trees * tree_bytes, tree_bytes / 4u, trees);
    }
}

} // namespace
