// ttt.hip -- batched n-player TicTacToe stepper for gfx950 (MI355X).  Hand-written HIP, wave64.
//
// Restates, for B independent games at once:
//   colosseumrl/envs/tictactoe/tictactoe_2p_env.py:139-169  new_state
//   colosseumrl/envs/tictactoe/tictactoe_2p_env.py:240-315  next_state   (3p/4p files: same logic,
//   colosseumrl/envs/tictactoe/tictactoe_2p_env.py:317-348  valid_actions  other board shape / P)
//   WINNING_SHAPES: 2p:12-17, 3p:12-17, 4p:19-38
//
// Layout: a board has <= 32 cells, so each player's marks are ONE uint32 per game: occ[P][B].
// One lane per game; a wave reads 64 consecutive words per player (fully coalesced 256-B rows).
// Win test: the reference correlates the mover's mask with each line pattern in 'valid' mode,
// i.e. "some K-window along one of the 13 (3-D) / 4 (2-D) directions is fully the mover's".
// With the mask in a register that is K-1 shift-ANDs per direction against a per-direction
// start mask (windows that stay on the board).  Direction strides and start masks are
// wave-uniform kernel arguments (SGPRs) -- no table traffic at all.
#include "crl_common.hpp"
#include <cstdlib>
#include <type_traits>
#include <vector>

namespace {


// ND = 4 (boards with at most 4 line directions: everything 1-D / 2-D) or 13 (3-D).  Strides and start masks are plain
// SGPR operands and no direction needs its own branch (unused slots have start == 0).  A K-window along stride s is
// built by doubling: t = m & (m >> s) is "two in a row", t & (t >> 2s) four, ... -- for the pinned K = 3 / 4 / 5 that is
// two or three shift-and pairs per direction (K is wave-uniform: one scalar branch) where the plain K-1 rounds of the
// generic loop take K-1 pairs plus the copies that seed them.
// KC: K when the caller has branched on it already (3, 4, 5), else 0 = ask dd.K here.
template <int ND, int KC = 0>
__device__ __forceinline__ bool ttt_has_line(const ttt_dirs &dd, const uint32_t m)
{
    uint32_t hit = 0;
    const int K = KC ? KC : dd.K;
    if (K == 3) {
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const int s = dd.stride[d];
            hit |= m & (m >> s) & (m >> (2 * s)) & dd.start[d];
        }
    } else if (K == 4) {
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const int s = dd.stride[d];
            const uint32_t two = m & (m >> s);
            hit |= two & (two >> (2 * s)) & dd.start[d];
        }
    } else if (K == 5) {
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const int s = dd.stride[d];
            const uint32_t two = m & (m >> s);
            hit |= two & (two >> (2 * s)) & (m >> (4 * s)) & dd.start[d];
        }
    } else {
        uint32_t t[ND], run[ND];
#pragma unroll
        for (int d = 0; d < ND; ++d) t[d] = run[d] = m;
        for (int s = 1; s < K; ++s) {
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                t[d] >>= dd.stride[d];              // cell c + s * stride of direction d, seen from c
                run[d] &= t[d];
            }
        }
#pragma unroll
        for (int d = 0; d < ND; ++d) hit |= run[d] & dd.start[d];
    }
    return hit != 0;
}

// WT: test for a line by the win-mask table win_bits of a board of at most 16 cells (in LDS; crl_ttt_create builds it)
template <int P, int ND, bool WT = false>
__device__ __forceinline__ void ttt_step_core(const ttt_dirs &dd, uint32_t (&o)[P], int &winner, int &to_move,
                                              const int action, int &reward, int &term, int &winners,
                                              const uint32_t *win_bits = nullptr)
{
    const int pl = to_move;
    uint32_t all = 0, mine = 0;
#pragma unroll
    for (int p = 0; p < P; ++p) { all |= o[p]; mine = (p == pl) ? o[p] : mine; }
    // tictactoe_2p_env.py:293: non-empty action, target cell empty, no sticky winner
    const bool in_range = (action >= 0) & (action < dd.n_cells);
    const uint32_t bit = in_range ? (1u << (action & 31)) : 0u;
    const bool ok = in_range && !(all & bit) && winner < 0;
    if (ok) {
        mine |= bit;                                   // :295
        all |= bit;
#pragma unroll
        for (int p = 0; p < P; ++p) o[p] = (p == pl) ? mine : o[p];
        bool won;                                      // :296-300
        if constexpr (WT) {
            CRL_BOUNDS_LT(mine >> 5, 2048u, 203);
            won = ((win_bits[mine >> 5] >> (mine & 31u)) & 1u) != 0u;
        }
        else won = ttt_has_line<ND>(dd, mine);
        if (won) winner = pl;
    }
    reward = 0; term = 0; winners = -1;
    if (winner >= 0) {                                 // :302-308
        reward = (winner == pl) ? 1 : -1;
        winners = winner;
        term = 1;
    }
    if (all == dd.full) term = 1;                      // :310-311
    to_move = (pl + 1 == P) ? 0 : pl + 1;              // :313
}

// index of the r-th (0-based) set bit of m (row-major np.where order, tictactoe_2p_env.py:345): binary search over
// bit fields.  Per level: the count below the midpoint (bit-field extract + popcount), the rank moves on by an UNSIGNED
// min (r - c wraps to a huge value exactly when r < c), the position by a compare.
__device__ __forceinline__ int nth_set_bit(const uint32_t m, int r)
{
    // (Round 3 tried the decision of a level as a sign mask -- t = rr - c, neg = t >> 31 (arithmetic), pos |= w & ~neg --
    //  which keeps the chain off VCC and so saves the wait state (s_nop) each level's select needs behind the VALU write
    //  of VCC; but the mask costs a VALU instruction and lengthens the dependent chain: 1.107 -> 1.180 ms per 2048 plies.)
    uint32_t rr = (uint32_t)r, pos = 0, c;
    c = (uint32_t)__popc(m & 0xffffu);                              pos = (rr >= c) ? 16u : 0u;          rr = min(rr, rr - c);
    c = (uint32_t)__popc(__builtin_amdgcn_ubfe(m, pos, 8u));        pos = (rr >= c) ? pos + 8u : pos;    rr = min(rr, rr - c);
    c = (uint32_t)__popc(__builtin_amdgcn_ubfe(m, pos, 4u));        pos = (rr >= c) ? pos + 4u : pos;    rr = min(rr, rr - c);
    c = (uint32_t)__popc(__builtin_amdgcn_ubfe(m, pos, 2u));        pos = (rr >= c) ? pos + 2u : pos;    rr = min(rr, rr - c);
    c = __builtin_amdgcn_ubfe(m, pos, 1u);                          pos = (rr >= c) ? pos + 1u : pos;
    return (int)pos;
}

// The same search with its last three levels out of a table: [byte][rank] = position of the rank-th set bit of the byte,
// 2 KB of LDS filled by the 256 threads of the workgroup (ttt_fill_rank_table; the caller puts a __syncthreads behind it).
// Two levels by arithmetic find the byte, one LDS read the bit in it: 15 vector instructions + 1 LDS read where the
// five-level search takes 26 (in the rollout's ply, where this chain is a third of the instructions).
__device__ __forceinline__ uint2 ttt_rank_row(const uint32_t t)      // the eight bytes of row t (a byte value)
{
    uint32_t lo = 0, hi = 0, n = 0;
#pragma unroll
    for (uint32_t bit = 0; bit < 8; ++bit) {
        const bool set = (t >> bit) & 1u;
        const uint32_t v = set ? bit << ((n & 3u) * 8u) : 0u;
        lo |= (n < 4u) ? v : 0u;
        hi |= (n < 4u) ? 0u : v;
        n += set ? 1u : 0u;
    }
    return make_uint2(lo, hi);
}

__device__ __forceinline__ void ttt_fill_rank_table(uint8_t (&tab)[256 * 8])
{
    const uint32_t t = threadIdx.x & 255u;
    *reinterpret_cast<uint2 *>(&tab[t * 8]) = ttt_rank_row(t);
}

// SMALL: the board has at most 16 cells (3x3, 3x5): the first level falls away.
template <bool SMALL = false>
__device__ __forceinline__ uint32_t nth_set_bit_tab(const uint8_t (&tab)[256 * 8], const uint32_t m, const uint32_t r)
{
    uint32_t rr = r, pos = 0, c;
    if (!SMALL) { c = (uint32_t)__popc(m & 0xffffu);                pos = (rr >= c) ? 16u : 0u;          rr = min(rr, rr - c); }
    c = (uint32_t)__popc(__builtin_amdgcn_ubfe(m, pos, 8u));        pos = (rr >= c) ? pos + 8u : pos;    rr = min(rr, rr - c);
    CRL_BOUNDS_LT(rr, 8u, 201);                                  // the rank left for the byte table is a rank INSIDE that byte
    return pos + tab[__builtin_amdgcn_ubfe(m, pos, 8u) * 8u + rr];
}

// the random agent's 32-bit draw for the ply at step counter c of game g with n_empty empty cells (the RNG contract of
// ttt_rollout_kernel, stated there): the ply picks empty cell number hi32(draw * n_empty)
__device__ __forceinline__ uint32_t ttt_agent_word(const uint32_t g, const uint32_t c, const int n_empty, const uint32_t seed_lo,
                                                   const uint32_t seed_hi)
{
    const philox_out rnd = philox4x32_10<true>(g, c >> 3, 0u, CRL_TAG_TTT, seed_lo, seed_hi);
    const uint32_t sel = (c >> 1) & 3u;
    const uint32_t w = sel == 0 ? rnd.w[0] : sel == 1 ? rnd.w[1] : sel == 2 ? rnd.w[2] : rnd.w[3];
    return (c & 1u) ? w * (uint32_t)(n_empty + 1) : w;
}

// every player's marks
template <int P>
__device__ __forceinline__ uint32_t ttt_union(const uint32_t (&o)[P])
{
    uint32_t all = 0;
#pragma unroll
    for (int p = 0; p < P; ++p) all |= o[p];
    return all;
}

// the random agent's move at step counter c of game g on a board whose marks are `all`: empty cell number
// hi32(draw * n_empty) in row-major order, -1 (the pass) on a full board
__device__ __forceinline__ int ttt_agent_move(const uint32_t full, const uint32_t all, const uint32_t g, const uint32_t c,
                                              const uint32_t seed_lo, const uint32_t seed_hi)
{
    const uint32_t empty = full & ~all;
    const int n_empty = __popc(empty);
    return n_empty ? nth_set_bit(empty, (int)__umulhi(ttt_agent_word(g, c, n_empty, seed_lo, seed_hi), (uint32_t)n_empty)) : -1;
}

// the 8 KB win-mask table of a board of at most 16 cells from memory into LDS by the 256 threads of the workgroup, two
// uint4 each (the caller puts a __syncthreads behind it)
__device__ __forceinline__ void ttt_stage_win_table(uint32_t *win_bits, const uint32_t *__restrict__ win_tab)
{
    const uint4 *src = reinterpret_cast<const uint4 *>(win_tab);
    uint4 *dst = reinterpret_cast<uint4 *>(win_bits);
    dst[threadIdx.x] = src[threadIdx.x];
    dst[threadIdx.x + 256] = src[threadIdx.x + 256];
}

// ---- the tactical (win-or-block) agent's two helpers; the contract is in include/colosseum_hip.h.  Used by the
// ttt_*_tactical kernels and ttt_winning_cells_kernel only.
//
// The empty cells e of E with "m | 1 << e holds a K-line" for a player's marks m (m and E are disjoint).  Per direction and
// window offset j the windows whose OTHER K - 1 cells are all in m are start & AND_{i != j} (m >> i s); their completing
// cell is offset j, so the mask goes back up by j s.  K = 3, 4, 5 (K is wave-uniform: one scalar branch) share the partial
// ANDs between the offsets.  Any other K counts instead: a window that lies in m | E and holds exactly one cell of E
// (`one` = some cell, `two` = two or more) is completed by that cell -- two passes of K shift-ANDs, no per-offset array.
// (Boards of at most 16 cells could look each empty cell up in the win-mask table instead: measured, that is slower --
// DESIGN.md 4.5b.)  A used direction has (K - 1) s <= 31 (its windows stay on the board); an unused slot (ND above
// n_dirs) has stride 0 and start 0, so no shift count ever reaches 32.  A player who HOLDS a line already (`hit`; no
// state of a game that records its winner, but a hand-made one) wins with whatever it adds: every empty cell.
template <int ND>
__device__ __forceinline__ uint32_t ttt_winning_cells(const ttt_dirs &dd, const uint32_t m, const uint32_t E)
{
    uint32_t cells = 0, hit = 0;
    const int K = dd.K;
    if (K == 3) {
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const int s = dd.stride[d];
            const uint32_t st = dd.start[d], a1 = m >> s, a2 = m >> (2 * s), lo = st & m & a1;
            cells |= (st & a1 & a2) | ((st & m & a2) << s) | (lo << (2 * s));
            hit |= lo & a2;
        }
    } else if (K == 4) {
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const int s = dd.stride[d];
            const uint32_t st = dd.start[d], a1 = m >> s, a2 = m >> (2 * s), a3 = m >> (3 * s);
            const uint32_t lo = st & m & a1, hi = st & a2 & a3;
            cells |= (a1 & hi) | ((m & hi) << s) | ((lo & a3) << (2 * s)) | ((lo & a2) << (3 * s));
            hit |= lo & hi;
        }
    } else if (K == 5) {
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const int s = dd.stride[d];
            const uint32_t st = dd.start[d], a1 = m >> s, a2 = m >> (2 * s), a3 = m >> (3 * s), a4 = m >> (4 * s);
            const uint32_t lo = st & m & a1, hi = a3 & a4, lo3 = lo & a2, hi3 = st & a2 & hi;
            cells |= (a1 & hi3) | ((m & hi3) << s) | ((lo & hi) << (2 * s)) | ((lo3 & a4) << (3 * s)) | ((lo3 & a3) << (4 * s));
            hit |= lo3 & hi;
        }
    } else {
        const uint32_t me = m | E;
        uint32_t in[ND], one[ND], two[ND];
#pragma unroll
        for (int d = 0; d < ND; ++d) { in[d] = me; one[d] = E; two[d] = 0u; }
        for (int i = 1; i < K; ++i) {
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                const int sh = i * dd.stride[d];
                const uint32_t e = E >> sh;
                in[d] &= me >> sh;
                two[d] |= one[d] & e;
                one[d] |= e;
            }
        }
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            in[d] &= dd.start[d];
            hit |= in[d] & ~one[d];                                                // a window without a cell of E: a line
            in[d] &= one[d] & ~two[d];                                             // the windows one cell short of a line
        }
        for (int i = 0; i < K; ++i) {
#pragma unroll
            for (int d = 0; d < ND; ++d) cells |= in[d] << (i * dd.stride[d]);     // (every cell of them; & E keeps the empty one)
        }
    }
    return hit ? E : cells & E;
}

// the tactical agent's Philox block for step counter c of game g: one block serves the two plies 2 (c >> 1) and 2 (c >> 1) + 1
// (c2 = 0 and CRL_TAG_TTT_TACTICAL, or (a << 16) | r and CRL_TAG_TTT_TACTICAL_PLAYOUT in a playout)
__device__ __forceinline__ philox_out ttt_tactical_block(const uint32_t g, const uint32_t c, const uint32_t c2, const uint32_t tag,
                                                         const uint32_t seed_lo, const uint32_t seed_hi)
{
    return philox4x32_10<true>(g, c >> 1, c2, tag, seed_lo, seed_hi);
}

// the tactical agent's move for the mover tm at step counter c, `rnd` the block of c: -1 (pass) without a mover or an empty
// cell; else word 2 (c & 1) decides "noisy" (below thr) and the next word picks a cell of S -- all empty cells on a noisy
// ply, else the first non-empty set of winning cells of the players tm, tm + 1, ... in turn order (its own win, then the
// earliest threat), all empty cells when nobody has one.  The cascade stops at the first non-empty set (per lane).
template <int P, int ND>
__device__ __forceinline__ int ttt_tactical_move(const ttt_dirs &dd, const uint32_t (&o)[P], const int tm, const philox_out &rnd,
                                                 const uint32_t c, const uint64_t thr)
{
    const uint32_t E = dd.full & ~ttt_union<P>(o);
    if ((unsigned)tm >= (unsigned)P || E == 0u) return -1;
    const uint32_t u = (c & 1u) ? rnd.w[2] : rnd.w[0], v = (c & 1u) ? rnd.w[3] : rnd.w[1];
    uint32_t S = E;
    if ((uint64_t)u >= thr) {
        int q = tm;
#pragma unroll 1
        for (int i = 0; i < P; ++i) {
            uint32_t m = 0;
#pragma unroll
            for (int p = 0; p < P; ++p) m = (p == q) ? o[p] : m;
            const uint32_t W = ttt_winning_cells<ND>(dd, m, E);
            if (W) { S = W; break; }
            q = (q + 1 == P) ? 0 : q + 1;
        }
    }
    return nth_set_bit(S, (int)__umulhi(v, (uint32_t)__popc(S)));
}

// Everything above, and the dispatch macros behind the kernels, is what ttt_puct.hip builds its kernels from: it includes
// this file with TTT_DEVICE_ONLY set and takes neither the kernels nor the entries.  That search is a translation unit of
// its own so that the kernels below compile to what they compile to without it.
#ifndef TTT_DEVICE_ONLY

template <int P, int ND>
__global__ void __launch_bounds__(256)
ttt_step_kernel(const ttt_dirs dd, const int64_t B, uint32_t *__restrict__ occ, int8_t *__restrict__ winner,
                int8_t *__restrict__ to_move, const int8_t *__restrict__ action, int8_t *__restrict__ reward,
                uint8_t *__restrict__ terminal, int8_t *__restrict__ winners, const uint32_t flags)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    uint32_t o[P];
#pragma unroll
    for (int p = 0; p < P; ++p) o[p] = occ[p * B + b];
    int w = winner[b], tm = to_move[b], r, t, ws;
    ttt_step_core<P, ND>(dd, o, w, tm, action[b], r, t, ws);
    reward[b] = (int8_t)r;
    terminal[b] = (uint8_t)t;
    winners[b] = (int8_t)ws;
    if (t && (flags & CRL_STEP_AUTO_RESET)) {
#pragma unroll
        for (int p = 0; p < P; ++p) o[p] = 0;
        w = -1; tm = 0;
    }
#pragma unroll
    for (int p = 0; p < P; ++p) occ[p * B + b] = o[p];
    winner[b] = (int8_t)w;
    to_move[b] = (int8_t)tm;
}

// WT: the board has at most 16 cells and win_tab is its table of winning masks (crl_ttt_create); ND = 4 then
template <int P, int ND, bool WT = false>
__global__ void __launch_bounds__(256)
ttt_rollout_kernel(const ttt_dirs dd, const int64_t B, const uint32_t seed_lo, const uint32_t seed_hi,
                   const uint64_t first_env_id, const int T, uint32_t *__restrict__ occ,
                   int8_t *__restrict__ winner, int8_t *__restrict__ to_move, const crl_ttt_stats st,
                   const uint32_t *__restrict__ win_tab)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    __shared__ uint8_t rank_tab[256 * 8];
    __shared__ uint32_t win_bits[WT ? 2048 : 1];             // boards of <= 16 cells: bit m = the mask m holds a K-line
    ttt_fill_rank_table(rank_tab);
    if (WT) ttt_stage_win_table(win_bits, win_tab);
    __syncthreads();
    if (b >= B) return;
    uint32_t o[P], wins[P];
#pragma unroll
    for (int p = 0; p < P; ++p) { o[p] = occ[p * B + b]; wins[p] = 0; }
    int w = winner[b], tm = to_move[b];
    uint32_t tc = st.tcount[b], ts = st.tstep[b], n_ep = 0, draws = 0, len_sum = 0;
    const uint32_t g = (uint32_t)(first_env_id + (uint64_t)b);
    // RNG contract (round 3, identical in the oracle): one Philox call serves EIGHT plies, a 32-bit word two -- block
    // tc >> 3, word (tc >> 1) & 3.  The ply at an even step counter reads the word w itself, the ply at an odd one
    // lo32(w * (n_empty + 1)): what the even ply's extraction hi32(w * n) left over when that ply was the one before in the
    // same game (n = n_empty + 1 then; the two choices are the leading digits of w in the mixed radix (n, n - 1), bias
    // < n^2 / 2^32).  The definition does not look back, so any ply follows from (seed, game, step counter, board) alone.
    // Round 2 drew one word per ply: the ten Philox rounds were 36 % of a ply's vector instructions.
    philox_out rnd = philox4x32_10<true>(g, tc >> 3, 0u, CRL_TAG_TTT, seed_lo, seed_hi);
    // one ply with the Philox word `pw` of its step counter (odd: that counter is odd)
    auto ply = [&](const uint32_t pw, const uint32_t odd) {
        uint32_t all = 0;
#pragma unroll
        for (int p = 0; p < P; ++p) all |= o[p];
        const uint32_t empty = dd.full & ~all;
        const int n_empty = __popc(empty);
        const uint32_t word = odd ? pw * (uint32_t)(n_empty + 1) : pw;
        const int action = n_empty ? nth_set_bit(empty, (int)__umulhi(word, (uint32_t)n_empty)) : -1;
        int r, term, ws;
        ttt_step_core<P, ND>(dd, o, w, tm, action, r, term, ws);
        ts += 1;
        if (term) {
            n_ep += 1;
            len_sum += ts;
            draws += (ws < 0);
#pragma unroll
            for (int p = 0; p < P; ++p) { wins[p] += (ws == p); o[p] = 0; }
            w = -1; tm = 0; ts = 0;
        }
    };
    // The same ply for a game that is RUNNING when the ply starts (no sticky winner, board not full) -- which every game is
    // once it has been through a ply of this kernel, because a finished game restarts at once: the random agent's move
    // is legal by construction, so next_state's checks (in range, cell empty, no winner yet: tictactoe_2p_env.py:293) and
    // the empty-board-is-full corner fall away, and the winner is known the moment the line test says so.
    // Round 3: the players' masks ROTATE through the registers r[] -- r[0] is always the mover's, because the players move
    // in strict rotation (:313) and a restart empties every mask, so that the rotation's phase means nothing across it.
    // The mover's mask then costs no select chain (round 2: P compares, 2 P selects and an or3 per ply) and, the plies
    // being unrolled, the rotation itself is register renaming.  Episode lengths are not summed per episode either: the
    // lengths of the episodes a lane finished add up to the plies it played minus the length of the unfinished one, so
    // a lane only remembers where its current episode began (ep0, a ply index of this launch).  And the outcomes are
    // counted in ONE register of byte fields -- field p the wins of player p, field P the draws (P = 8: the draws are the
    // episodes nobody won) -- which a finished episode bumps with a select, a shift and an add (per-player counters: a
    // compare, a select and an add EACH, in the block some lane of the wave runs on practically every ply); the fields are
    // flushed into the 32-bit counters before any can reach 256, i.e. at least every 248 plies.
    uint32_t all_run = 0;                                       // every player's marks (kept across running plies)
    uint32_t r[P];
    int ep0 = 0;                                                // ply index (of this launch) at which the current episode began
    constexpr bool DRAW_FIELD = P < 8;
    using acc_t = std::conditional_t<(P <= 3), uint32_t, uint64_t>;
    acc_t acc = 0;
    int tm8 = 0;                                                // 8 * (player to move) while the running plies are at it
    auto flush = [&]() {
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const uint32_t f = (uint32_t)(acc >> (8 * p)) & 0xffu;
            wins[p] += f;
            n_ep += f;
        }
        if (DRAW_FIELD) {
            const uint32_t f = (uint32_t)(acc >> (8 * (P & 7))) & 0xffu;
            draws += f;
            n_ep += f;
        }
        acc = 0;
    };
    auto ply_running = [&](auto k_tag, const uint32_t w, const uint32_t odd, const int t_after) {   // k_tag: K as a compile-time constant (0: read it from dd)
        constexpr int KC = decltype(k_tag)::value & 7;            // k_tag: K (0: read it from dd) | 8 for boards of <= 16 cells
        constexpr bool SMALL = (decltype(k_tag)::value & 8) != 0;  //        | 16: ... whose win test is a table lookup
        constexpr bool TABLE = WT && (decltype(k_tag)::value & 16) != 0;
        const uint32_t empty = dd.full & ~all_run;              // (not 0: the game is running)
        const uint32_t n_empty = (uint32_t)__popc(empty);
        const uint32_t word = odd ? w * (n_empty + 1u) : w;     // (odd is a constant in the unrolled trips)
        const uint32_t bit = 1u << nth_set_bit_tab<SMALL>(rank_tab, empty, __umulhi(word, n_empty));
        const uint32_t mine = r[0] | bit;                                              // :295
        bool won;                                                                      // :296-300
        if constexpr (TABLE) {
            CRL_BOUNDS_LT(mine >> 5, 2048u, 202);               // masks of boards with at most 16 cells
            won = ((win_bits[mine >> 5] >> (mine & 31u)) & 1u) != 0u;
        }
        else won = ttt_has_line<ND, KC>(dd, mine);
        all_run |= bit;
        const bool term = won | (all_run == dd.full);                                  // :302-311
#pragma unroll
        for (int p = 0; p + 1 < P; ++p) r[p] = r[p + 1];
        r[P - 1] = mine;
        const int pl8 = tm8;
        if constexpr (P <= 4) {                                                        // :313: the next mover out of a constant of
            constexpr uint32_t kNext = P == 1 ? 0u : P == 2 ? 0x0008u : P == 3 ? 0x001008u : 0x00181008u;   // bytes (one v_bfe)
            tm8 = (int)__builtin_amdgcn_ubfe(kNext, (uint32_t)pl8, 8u);
        } else {
            tm8 = (pl8 + 8 == 8 * P) ? 0 : pl8 + 8;
        }
        // (The end of an episode as selects instead of a branch -- some lane of the wave ends one on practically every ply
        //  -- is a wash: +0.7 % at 5x5, -2.3 % at 3x3x3; the selects cost 6 more vector instructions per ply.)
        if (term) {
            if (DRAW_FIELD) {
                acc += (acc_t)1 << (won ? pl8 : 8 * P);
            } else {
                acc += (acc_t)(won ? 1u : 0u) << pl8;
                draws += won ? 0u : 1u;
                n_ep += won ? 0u : 1u;
            }
#pragma unroll
            for (int p = 0; p < P; ++p) r[p] = 0;
            tm8 = 0; all_run = 0; ep0 = t_after;
        }
    };
    auto next_word = [&](uint32_t &odd) -> uint32_t {           // the word of step counter tc, then on to tc + 1
        const uint32_t sel = (tc >> 1) & 3u;
        odd = tc & 1u;
        uint32_t word = rnd.w[0];
        word = (sel == 1) ? rnd.w[1] : word;
        word = (sel == 2) ? rnd.w[2] : word;
        word = (sel == 3) ? rnd.w[3] : word;
        tc += 1;
        if ((tc & 7u) == 0) rnd = philox4x32_10<true>(g, tc >> 3, 0u, CRL_TAG_TTT, seed_lo, seed_hi);
        return word;
    };
    int t = 0;
    {   // a state that came in finished but not restarted (stepped without auto-reset, or hand-made): one general ply
        uint32_t all = 0;
#pragma unroll
        for (int p = 0; p < P; ++p) all |= o[p];
        if (T > 0 && __builtin_amdgcn_ballot_w64(w >= 0 || all == dd.full || (unsigned)tm >= (unsigned)P) != 0ull) {
            uint32_t odd;
            const uint32_t w0 = next_word(odd);
            ply(w0, odd);
            t = 1;
        }
    }
    // into the rotating order: r[i] = the marks of player (tm + i) mod P
    const int tm_in = (unsigned)tm < (unsigned)P ? tm : 0;
#pragma unroll
    for (int i = 0; i < P; ++i) {
        int q = tm_in + i;
        q = q >= P ? q - P : q;
        uint32_t v = 0;
#pragma unroll
        for (int p = 0; p < P; ++p) { v = (q == p) ? o[p] : v; }
        r[i] = v;
        all_run |= v;
    }
    tm8 = 8 * tm_in;
    ep0 = t - (int)ts;                                          // the current episode is ts plies old
    const int ep0_in = ep0;
    // When every game of the wave stands at a step counter that is a multiple of eight (launches of 8 k steps keep it so)
    // the plies run in trips of eight -- one Philox call -- with word and parity picked at compile time: no per-ply select
    // chain, no refill test.
    // (K is wave-uniform: one branch here instead of one per ply)
    auto run_plies = [&](auto k_tag) {
        if (__builtin_amdgcn_ballot_w64((tc & 7u) != 0u) == 0ull) {
            for (int trips = 0; t + 8 <= T; t += 8) {
                if (++trips == 32) { flush(); trips = 1; }      // <= 31 trips = 248 plies between flushes
                ply_running(k_tag, rnd.w[0], 0u, t + 1);
                ply_running(k_tag, rnd.w[0], 1u, t + 2);
                ply_running(k_tag, rnd.w[1], 0u, t + 3);
                ply_running(k_tag, rnd.w[1], 1u, t + 4);
                ply_running(k_tag, rnd.w[2], 0u, t + 5);
                ply_running(k_tag, rnd.w[2], 1u, t + 6);
                ply_running(k_tag, rnd.w[3], 0u, t + 7);
                ply_running(k_tag, rnd.w[3], 1u, t + 8);
                tc += 8;
                rnd = philox4x32_10<true>(g, tc >> 3, 0u, CRL_TAG_TTT, seed_lo, seed_hi);
            }
        }
        flush();
        for (; t < T; ++t) {
            uint32_t odd;
            const uint32_t w1 = next_word(odd);
            ply_running(k_tag, w1, odd, t + 1);
            if ((t & 127) == 127) flush();
        }
        flush();
    };
    if constexpr (WT) {
        run_plies(std::integral_constant<int, 8 | 16>{});        // 3x3, 3x5 (the reference's 2p / 3p boards), 4x4, ...
    } else {
        if (dd.K == 3 && dd.n_cells <= 16) run_plies(std::integral_constant<int, 3 | 8>{});
        else if (dd.K == 3) run_plies(std::integral_constant<int, 3>{});
        else if (dd.K == 4) run_plies(std::integral_constant<int, 4>{});
        else run_plies(std::integral_constant<int, 0>{});
    }
    // back out of the rotating order, and the bookkeeping the running plies left implicit
    {
        tm = tm8 >> 3;
        const int tm_out = tm;
#pragma unroll
        for (int p = 0; p < P; ++p) {
            int i = p - tm_out;
            i = i < 0 ? i + P : i;
            uint32_t v = 0;
#pragma unroll
            for (int k = 0; k < P; ++k) { v = (i == k) ? r[k] : v; }
            o[p] = v;
        }
        ts = (uint32_t)(T - ep0);                               // plies of the unfinished episode
        len_sum += (uint32_t)(ep0 - ep0_in);                    // = the lengths of the episodes finished by running plies
    }
    int32_t *row = st.results ? st.results + b * (3 + P) : nullptr;    // packed result row for the gather
#pragma unroll
    for (int p = 0; p < P; ++p) {
        occ[p * B + b] = o[p];
        const uint32_t wc = st.win_count[p * B + b] + wins[p];
        st.win_count[p * B + b] = wc;
        if (row) row[3 + p] = (int32_t)wc;
    }
    winner[b] = (int8_t)w;
    to_move[b] = (int8_t)tm;
    st.tcount[b] = tc;
    st.tstep[b] = ts;
    const uint32_t ne = st.n_episodes[b] + n_ep, dr = st.draw_count[b] + draws, ls = st.len_sum[b] + len_sum;
    st.n_episodes[b] = ne;
    st.draw_count[b] = dr;
    st.len_sum[b] = ls;
    if (row) { row[0] = (int32_t)ne; row[1] = (int32_t)ls; row[2] = (int32_t)dr; }
}

// int8 [B][cells] boards of the 256 games of a workgroup from their occupancy masks in LDS: -1 empty, else the owner's
// id -- relative to s_rel[game] when that is >= 0 (_relative_player_id, tictactoe_2p_env.py:26-27: python's non-negative
// modulo by rel_mod).  One dword (four cells) per thread and trip, written coalesced; the bytes of a workgroup start at
// a multiple of 256 * cells, so dword stores are aligned whenever the buffer is.
template <int P>
__device__ __forceinline__ void ttt_write_boards(const uint32_t (&s_occ)[P][256], const int (&s_rel)[256], const int cells,
                                                 const uint32_t inv_cells, const int rel_mod, const int64_t g0, const int64_t B,
                                                 int8_t *__restrict__ obs)
{
    const int n_game = (int)((B - g0) < 256 ? (B - g0) : 256);
    const int total = n_game * cells;
    int8_t *out = obs + g0 * cells;
    for (int d = threadIdx.x; d * 4 < total; d += 256) {
        int e = cells == 1 ? d * 4 : (int)__umulhi((uint32_t)(d * 4), inv_cells);
        int c = d * 4 - e * cells;
        uint32_t word = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ee = e < 256 ? e : 255;       // bytes past the last game of the block are never stored
            int v = -1;
#pragma unroll
            for (int p = 0; p < P; ++p) v = ((s_occ[p][ee] >> c) & 1u) ? p : v;
            const int rel = s_rel[ee];
            if (v >= 0 && rel >= 0) {
                const int rr = (v - rel) % rel_mod;
                v = rr < 0 ? rr + rel_mod : rr;
            }
            word |= (uint32_t)(v & 0xff) << (8 * k);
            if (++c == cells) { c = 0; ++e; }
        }
        if (d * 4 + 4 <= total) {
            *reinterpret_cast<uint32_t *>(out + d * 4) = word;
        } else {
            for (int k = 0; d * 4 + k < total; ++k) out[d * 4 + k] = (int8_t)(word >> (8 * k));
        }
    }
}

// ---- fused per-step call: [sample ->] next_state (auto-reset) -> valid_actions mask + state_to_observation of the
// player to move next.  What a learner / vector env runs every ply (tictactoe_2p_env.py:240-315, :317-348, :382-407);
// as separate launches (crl_ttt_sample, crl_ttt_step, crl_ttt_valid, crl_ttt_board) the launch boundaries cost more than
// the work.  One lane per game plays the move; the post-move masks go through LDS so that the int8 [B][cells] observation
// is produced a dword per thread and written coalesced (a lane writing its own game's 9..27 bytes would not be).
template <int P, int ND>
__global__ void __launch_bounds__(256)
ttt_step_observe_kernel(const ttt_dirs dd, const uint32_t inv_cells, const int64_t B, const uint32_t seed_lo,
                        const uint32_t seed_hi, const uint64_t first_env_id, uint32_t *__restrict__ occ,
                        int8_t *__restrict__ winner, int8_t *__restrict__ to_move, const int8_t *__restrict__ action,
                        uint32_t *__restrict__ tcount, int8_t *__restrict__ reward, uint8_t *__restrict__ terminal,
                        int8_t *__restrict__ winners, int8_t *__restrict__ obs, uint32_t *__restrict__ valid,
                        const int rel_mod, const uint32_t flags)
{
    __shared__ uint32_t s_occ[P][256];
    __shared__ int s_mover[256];
    const int64_t g0 = (int64_t)blockIdx.x * 256;
    const int64_t b = g0 + threadIdx.x;
    uint32_t o[P];
    int tm = 0;
#pragma unroll
    for (int p = 0; p < P; ++p) o[p] = 0u;
    if (b < B) {
#pragma unroll
        for (int p = 0; p < P; ++p) o[p] = occ[p * B + b];
        int w = winner[b];
        tm = to_move[b];
        int act;
        if (action) {
            act = action[b];
        } else {                                    // the rollout's random agent at this game's step counter
            const uint32_t c = tcount[b];
            act = ttt_agent_move(dd.full, ttt_union<P>(o), (uint32_t)(first_env_id + (uint64_t)b), c, seed_lo, seed_hi);
            tcount[b] = c + 1u;
        }
        int r, t, ws;
        ttt_step_core<P, ND>(dd, o, w, tm, act, r, t, ws);
        reward[b] = (int8_t)r;
        terminal[b] = (uint8_t)t;
        winners[b] = (int8_t)ws;
        if (t && (flags & CRL_STEP_AUTO_RESET)) {
#pragma unroll
            for (int p = 0; p < P; ++p) o[p] = 0;
            w = -1; tm = 0;
        }
        uint32_t all = 0;
#pragma unroll
        for (int p = 0; p < P; ++p) { occ[p * B + b] = o[p]; all |= o[p]; }
        winner[b] = (int8_t)w;
        to_move[b] = (int8_t)tm;
        valid[b] = dd.full & ~all;                  // tictactoe_2p_env.py:317-348 for the player to move next
    }
#pragma unroll
    for (int p = 0; p < P; ++p) s_occ[p][threadIdx.x] = o[p];
    s_mover[threadIdx.x] = tm;
    __syncthreads();
    ttt_write_boards<P>(s_occ, s_mover, dd.n_cells, inv_cells, rel_mod, g0, B, obs);
}

// ---- one learner against the random agent (crl_ttt_step_single; the contract is in include/colosseum_hip.h): per game
// an optional learner ply, then the random agent for every other seat until it is the learner's turn again -- across the
// end of a game and its restart -- and the learner's valid mask and observation of what that leaves.  One lane per game,
// the plies a per-lane loop of at most 1 + 2 (P - 1) trips over ttt_step_core (the same ply as crl_ttt_step); the draws are
// crl_ttt_sample's.  Boards of at most 16 cells take the win test out of the win-mask table (WT), staged into LDS as the
// rollout does.  The observation goes through LDS as in ttt_step_observe_kernel.
template <int P, int ND, bool WT>
__global__ void __launch_bounds__(256)
ttt_step_single_kernel(const ttt_dirs dd, const uint32_t inv_cells, const int64_t B, const uint32_t seed_lo,
                       const uint32_t seed_hi, const uint64_t first_env_id, uint32_t *__restrict__ occ,
                       int8_t *__restrict__ winner, int8_t *__restrict__ to_move, const int8_t *__restrict__ seat,
                       const int64_t *__restrict__ learner_action, uint32_t *__restrict__ tcount,
                       int8_t *__restrict__ reward, uint8_t *__restrict__ done, int8_t *__restrict__ winners,
                       int8_t *__restrict__ obs, uint32_t *__restrict__ valid, const int rel_mod,
                       const uint32_t *__restrict__ win_tab)
{
    __shared__ uint32_t s_occ[P][256];
    __shared__ int s_seat[256];
    __shared__ uint32_t win_bits[WT ? 2048 : 1];
    if (WT) {
        ttt_stage_win_table(win_bits, win_tab);
        __syncthreads();
    }
    const int64_t g0 = (int64_t)blockIdx.x * 256;
    const int64_t b = g0 + threadIdx.x;
    uint32_t o[P];
    int s = 0;
#pragma unroll
    for (int p = 0; p < P; ++p) o[p] = 0u;
    if (b < B) {
#pragma unroll
        for (int p = 0; p < P; ++p) o[p] = occ[p * B + b];
        int w = winner[b], tm = to_move[b];
        s = (int)seat[b] % P;
        s += s < 0 ? P : 0;
        uint32_t c = tcount[b];
        const uint32_t g = (uint32_t)(first_env_id + (uint64_t)b);
        int rew = 0, dn = 0, wout = -1;
        bool learner = learner_action != nullptr && tm == s;
        for (int opp = 0; learner || (tm != s && opp < 2 * (P - 1)); ) {
            int act;
            if (learner) {                          // crl_ttt_step's int8 action for v in [-1, cells), else the pass
                const int64_t v = learner_action[b];
                act = (v >= -1 && v < dd.n_cells) ? (int)v : -1;
            } else {                                // crl_ttt_sample at this game's step counter
                act = ttt_agent_move(dd.full, ttt_union<P>(o), g, c, seed_lo, seed_hi);
                ++opp;
            }
            c += 1u;
            learner = false;
            int r, t, ws;
            ttt_step_core<P, ND, WT>(dd, o, w, tm, act, r, t, ws, win_bits);
            if (t) {                                // the learner's outcome (current_rewards, tictactoe_2p_env.py:233-236), restart
                dn = 1;
                wout = ws;
                rew = ws < 0 ? 0 : (ws == s ? 1 : -1);
#pragma unroll
                for (int p = 0; p < P; ++p) o[p] = 0;
                w = -1; tm = 0;
            }
        }
        uint32_t all = 0;
#pragma unroll
        for (int p = 0; p < P; ++p) { occ[p * B + b] = o[p]; all |= o[p]; }
        winner[b] = (int8_t)w;
        to_move[b] = (int8_t)tm;
        tcount[b] = c;
        reward[b] = (int8_t)rew;
        done[b] = (uint8_t)dn;
        winners[b] = (int8_t)wout;
        valid[b] = dd.full & ~all;
    }
#pragma unroll
    for (int p = 0; p < P; ++p) s_occ[p][threadIdx.x] = o[p];
    s_seat[threadIdx.x] = s;
    __syncthreads();
    ttt_write_boards<P>(s_occ, s_seat, dd.n_cells, inv_cells, rel_mod, g0, B, obs);
}

// ---- batched random playouts (crl_ttt_playout; the contract is in include/colosseum_hip.h).  One lane per playout, the
// flat lane index i = (b * A + a) * R + r (r fastest): the lanes of one row are neighbours, so a row is one segment of a
// wave (R <= 64 and aligned) or spans several waves.  A lane loads its position (the R lanes of a row read the same words:
// cache hits), plays the candidate ply if there is one and then random plies until the first terminal one; the wave runs
// until its longest playout ends.  The draws are the rollout's agent under the playout tag and the third counter word
// (a << 16) | r: one Philox block per eight step counters, kept in registers and its word picked as the rollout's
// next_word does (ttt_agent_word would redo the ten rounds on every ply), the cell out of the rollout's rank table.  Outcomes leave through ballots: per row segment of the wave and output word, a popcount of the
// segment's bits (the plies as six bit planes), so that one head lane per segment issues one store -- or, for a row that
// also has lanes in other waves, one integer atomic onto the zeros the launcher wrote.
template <int P, int ND, bool WT>
__global__ void __launch_bounds__(256)
ttt_playout_kernel(const ttt_dirs dd, const int64_t B, const uint32_t seed_lo, const uint32_t seed_hi,
                   const uint64_t first_env_id, const uint32_t *__restrict__ occ, const int8_t *__restrict__ winner,
                   const int8_t *__restrict__ to_move, const uint32_t *__restrict__ tcount, const int32_t *__restrict__ cand,
                   const int A, const int R, const uint64_t n_lanes, uint32_t *__restrict__ wins,
                   uint32_t *__restrict__ played, uint32_t *__restrict__ len_sum, const uint32_t *__restrict__ win_tab)
{
    constexpr bool SMALL = WT;                                   // (WT: at most 16 cells)
    __shared__ uint8_t rank_tab[256 * 8];
    __shared__ uint32_t win_bits[WT ? 2048 : 1];
    ttt_fill_rank_table(rank_tab);
    if (WT) ttt_stage_win_table(win_bits, win_tab);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t wave0 = (uint64_t)blockIdx.x * 256u + (threadIdx.x & ~63u); wave0 < n_lanes; wave0 += stride) {
        // (b, a, r) of this lane: one 64-bit division per wave (wave-uniform), then a 32-bit one per lane
        const uint64_t row0 = wave0 / (uint32_t)R;
        const uint32_t r0 = (uint32_t)(wave0 - row0 * (uint32_t)R);
        const uint32_t q = (r0 + lane) / (uint32_t)R;
        const uint64_t row = row0 + q;
        const uint32_t r = r0 + lane - q * (uint32_t)R;
        const bool live = wave0 + lane < n_lanes;
        const int64_t b = live ? (int64_t)(row / (uint32_t)A) : 0;
        const uint32_t a = (uint32_t)(row - (uint64_t)b * (uint32_t)A);
        int wn = -1, len = 0;
        bool play = false;
        if (live) {
            uint32_t o[P], all = 0;
#pragma unroll
            for (int p = 0; p < P; ++p) { o[p] = occ[p * B + b]; all |= o[p]; }
            int w = winner[b], tm = to_move[b];
            play = w < 0 && all != dd.full && (unsigned)tm < (unsigned)P;   // a position that is over skips every row
            int first = -1;
            if (play && cand != nullptr) {                      // the candidate: an empty cell, else the row is skipped
                first = cand[b * A + a];
                play = first >= 0 && first < dd.n_cells && !((all >> (first & 31)) & 1u);
            }
            if (play) {
                const uint32_t g = (uint32_t)(first_env_id + (uint64_t)b), c2 = (a << 16) | r;
                uint32_t c = tcount ? tcount[b] : 0u;
                philox_out rnd = philox4x32_10<true>(g, c >> 3, c2, CRL_TAG_TTT_PLAYOUT, seed_lo, seed_hi);
                int term = 0, rw, ws = -1;
                if (first >= 0) {                               // the candidate ply: no draw
                    ttt_step_core<P, ND, WT>(dd, o, w, tm, first, rw, term, ws, win_bits);
                    len = 1;
                }
                while (!term) {                                 // random plies on a running game (the rollout's draw)
                    const uint32_t empty = dd.full & ~ttt_union<P>(o);
                    const uint32_t n_empty = (uint32_t)__popc(empty);           // (not 0: the game is running)
                    const uint32_t sel = (c >> 1) & 3u;
                    uint32_t word = rnd.w[0];
                    word = (sel == 1) ? rnd.w[1] : word;
                    word = (sel == 2) ? rnd.w[2] : word;
                    word = (sel == 3) ? rnd.w[3] : word;
                    word = (c & 1u) ? word * (n_empty + 1u) : word;
                    const int act = (int)nth_set_bit_tab<SMALL>(rank_tab, empty, __umulhi(word, n_empty));
                    ttt_step_core<P, ND, WT>(dd, o, w, tm, act, rw, term, ws, win_bits);
                    len += 1;
                    c += 1u;
                    if ((c & 7u) == 0u && !term) rnd = philox4x32_10<true>(g, c >> 3, c2, CRL_TAG_TTT_PLAYOUT, seed_lo, seed_hi);
                }
                wn = ws;
            }
        }
        // ---- per row segment of this wave: the lanes from a head (r == 0, or lane 0) to the next head
        const unsigned long long heads = __ballot(live && (lane == 0u || r == 0u));
        const unsigned long long above = lane == 63u ? 0ull : heads & (~0ull << (lane + 1u));
        const uint32_t end = above ? (uint32_t)__builtin_ctzll(above) : 64u;
        const unsigned long long seg = (end == 64u ? ~0ull : ((1ull << end) - 1ull)) & (~0ull << lane);
        const bool head = (heads >> lane) & 1ull;
        const bool whole = r == 0u && end - lane == (uint32_t)R;           // the row has no lane in another wave
        uint32_t cnt[P], n_played, plies = 0;
#pragma unroll
        for (int p = 0; p < P; ++p) cnt[p] = (uint32_t)__builtin_popcountll(__ballot(play && wn == p) & seg);
        n_played = (uint32_t)__builtin_popcountll(__ballot(play) & seg);
#pragma unroll
        for (int k = 0; k < 6; ++k)                              // len <= cells + 1 <= 33 < 2^6
            plies += (uint32_t)__builtin_popcountll(__ballot(play && ((len >> k) & 1)) & seg) << k;
        if (head) {
            if (whole) {
#pragma unroll
                for (int p = 0; p < P; ++p) wins[row * P + p] = cnt[p];
                played[row] = n_played;
                len_sum[row] = plies;
            } else if (n_played) {
#pragma unroll
                for (int p = 0; p < P; ++p)
                    if (cnt[p]) atomicAdd(&wins[row * P + p], cnt[p]);
                atomicAdd(&played[row], n_played);
                atomicAdd(&len_sum[row], plies);
            }
        }
    }
}

// the rollout's random agent for one step
__global__ void __launch_bounds__(256)
ttt_sample_kernel(const int P, const uint32_t full, const int64_t B, const uint32_t seed_lo, const uint32_t seed_hi,
                  const uint64_t first_env_id, const uint32_t *__restrict__ occ, uint32_t *__restrict__ tcount,
                  const int advance, int8_t *__restrict__ action)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    uint32_t all = 0;
    for (int p = 0; p < P; ++p) all |= occ[p * B + b];
    // ttt_agent_move's rule with the draw made BEFORE the test for a full board, as this kernel always had it: through the
    // helper (the draw behind the test) it compiles to 16 VGPRs / 20 SGPRs instead of 18 / 32, and a refactor that must
    // leave every kernel's registers alone cannot take that
    const uint32_t empty = full & ~all, c = tcount[b];
    const int n_empty = __popc(empty);
    const uint32_t word = ttt_agent_word((uint32_t)(first_env_id + (uint64_t)b), c, n_empty, seed_lo, seed_hi);
    action[b] = (int8_t)(n_empty ? nth_set_bit(empty, (int)__umulhi(word, (uint32_t)n_empty)) : -1);
    if (advance) tcount[b] = c + 1u;
}

// ---- the tactical agent's kernels (crl_ttt_winning_cells, crl_ttt_*_tactical): one lane per game (the playout: per
// playout).  The winning-cell sets are computed in every instance; the kernels that play plies test a ply's win out of the
// win-mask table of a board of at most 16 cells as their random siblings do (WT).
template <int P, int ND>
__global__ void __launch_bounds__(256)
ttt_winning_cells_kernel(const ttt_dirs dd, const int64_t B, const uint32_t *__restrict__ occ, uint32_t *__restrict__ cells)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    uint32_t o[P];
#pragma unroll
    for (int p = 0; p < P; ++p) o[p] = occ[p * B + b];
    const uint32_t E = dd.full & ~ttt_union<P>(o);
#pragma unroll
    for (int p = 0; p < P; ++p) cells[p * B + b] = ttt_winning_cells<ND>(dd, o[p], E);
}

template <int P, int ND>
__global__ void __launch_bounds__(256)
ttt_sample_tactical_kernel(const ttt_dirs dd, const int64_t B, const uint32_t seed_lo, const uint32_t seed_hi,
                           const uint64_t first_env_id, const uint64_t thr, const uint32_t *__restrict__ occ,
                           const int8_t *__restrict__ to_move, uint32_t *__restrict__ tcount, const int advance,
                           int8_t *__restrict__ action)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    uint32_t o[P];
#pragma unroll
    for (int p = 0; p < P; ++p) o[p] = occ[p * B + b];
    const uint32_t c = tcount[b];
    const philox_out rnd = ttt_tactical_block((uint32_t)(first_env_id + (uint64_t)b), c, 0u, CRL_TAG_TTT_TACTICAL, seed_lo, seed_hi);
    action[b] = (int8_t)ttt_tactical_move<P, ND>(dd, o, to_move[b], rnd, c, thr);
    if (advance) tcount[b] = c + 1u;
}

// T plies with every seat on the tactical agent: crl_ttt_rollout's general ply (ttt_step_core, the restart and the
// statistics of its `ply`) with the tactical move; the Philox block stays in registers for its two plies
template <int P, int ND, bool WT>
__global__ void __launch_bounds__(256)
ttt_rollout_tactical_kernel(const ttt_dirs dd, const int64_t B, const uint32_t seed_lo, const uint32_t seed_hi,
                            const uint64_t first_env_id, const uint64_t thr, const int T, uint32_t *__restrict__ occ,
                            int8_t *__restrict__ winner, int8_t *__restrict__ to_move, const crl_ttt_stats st,
                            const uint32_t *__restrict__ win_tab)
{
    __shared__ uint32_t win_bits[WT ? 2048 : 1];
    if (WT) {
        ttt_stage_win_table(win_bits, win_tab);
        __syncthreads();
    }
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    uint32_t o[P], wins[P];
#pragma unroll
    for (int p = 0; p < P; ++p) { o[p] = occ[p * B + b]; wins[p] = 0; }
    int w = winner[b], tm = to_move[b];
    uint32_t tc = st.tcount[b], ts = st.tstep[b], n_ep = 0, draws = 0, len_sum = 0;
    const uint32_t g = (uint32_t)(first_env_id + (uint64_t)b);
    philox_out rnd = ttt_tactical_block(g, tc, 0u, CRL_TAG_TTT_TACTICAL, seed_lo, seed_hi);
    for (int t = 0; t < T; ++t) {
        const int action = ttt_tactical_move<P, ND>(dd, o, tm, rnd, tc, thr);
        int r, term, ws;
        ttt_step_core<P, ND, WT>(dd, o, w, tm, action, r, term, ws, win_bits);
        ts += 1;
        tc += 1;
        if ((tc & 1u) == 0u) rnd = ttt_tactical_block(g, tc, 0u, CRL_TAG_TTT_TACTICAL, seed_lo, seed_hi);
        if (term) {
            n_ep += 1;
            len_sum += ts;
            draws += (ws < 0);
#pragma unroll
            for (int p = 0; p < P; ++p) { wins[p] += (ws == p); o[p] = 0; }
            w = -1; tm = 0; ts = 0;
        }
    }
    int32_t *row = st.results ? st.results + b * (3 + P) : nullptr;    // packed result row, as crl_ttt_rollout writes it
#pragma unroll
    for (int p = 0; p < P; ++p) {
        occ[p * B + b] = o[p];
        const uint32_t wc = st.win_count[p * B + b] + wins[p];
        st.win_count[p * B + b] = wc;
        if (row) row[3 + p] = (int32_t)wc;
    }
    winner[b] = (int8_t)w;
    to_move[b] = (int8_t)tm;
    st.tcount[b] = tc;
    st.tstep[b] = ts;
    const uint32_t ne = st.n_episodes[b] + n_ep, dr = st.draw_count[b] + draws, ls = st.len_sum[b] + len_sum;
    st.n_episodes[b] = ne;
    st.draw_count[b] = dr;
    st.len_sum[b] = ls;
    if (row) { row[0] = (int32_t)ne; row[1] = (int32_t)ls; row[2] = (int32_t)dr; }
}

// one learner against the tactical agent: ttt_step_single_kernel with the opponents' plies from ttt_tactical_move
template <int P, int ND, bool WT>
__global__ void __launch_bounds__(256)
ttt_step_single_tactical_kernel(const ttt_dirs dd, const uint32_t inv_cells, const int64_t B, const uint32_t seed_lo,
                                const uint32_t seed_hi, const uint64_t first_env_id, const uint64_t thr,
                                uint32_t *__restrict__ occ, int8_t *__restrict__ winner, int8_t *__restrict__ to_move,
                                const int8_t *__restrict__ seat, const int64_t *__restrict__ learner_action,
                                uint32_t *__restrict__ tcount, int8_t *__restrict__ reward, uint8_t *__restrict__ done,
                                int8_t *__restrict__ winners, int8_t *__restrict__ obs, uint32_t *__restrict__ valid,
                                const int rel_mod, const uint32_t *__restrict__ win_tab)
{
    __shared__ uint32_t s_occ[P][256];
    __shared__ int s_seat[256];
    __shared__ uint32_t win_bits[WT ? 2048 : 1];
    if (WT) {
        ttt_stage_win_table(win_bits, win_tab);
        __syncthreads();
    }
    const int64_t g0 = (int64_t)blockIdx.x * 256;
    const int64_t b = g0 + threadIdx.x;
    uint32_t o[P];
    int s = 0;
#pragma unroll
    for (int p = 0; p < P; ++p) o[p] = 0u;
    if (b < B) {
#pragma unroll
        for (int p = 0; p < P; ++p) o[p] = occ[p * B + b];
        int w = winner[b], tm = to_move[b];
        s = (int)seat[b] % P;
        s += s < 0 ? P : 0;
        uint32_t c = tcount[b];
        const uint32_t g = (uint32_t)(first_env_id + (uint64_t)b);
        int rew = 0, dn = 0, wout = -1;
        bool learner = learner_action != nullptr && tm == s, have = false;
        philox_out rnd = {};
        for (int opp = 0; learner || (tm != s && opp < 2 * (P - 1)); ) {
            int act;
            if (learner) {                          // crl_ttt_step's int8 action for v in [-1, cells), else the pass
                const int64_t v = learner_action[b];
                act = (v >= -1 && v < dd.n_cells) ? (int)v : -1;
            } else {                                // crl_ttt_sample_tactical at this game's step counter
                if (!have || (c & 1u) == 0u) rnd = ttt_tactical_block(g, c, 0u, CRL_TAG_TTT_TACTICAL, seed_lo, seed_hi);
                have = true;
                act = ttt_tactical_move<P, ND>(dd, o, tm, rnd, c, thr);
                ++opp;
            }
            c += 1u;
            learner = false;
            int r, t, ws;
            ttt_step_core<P, ND, WT>(dd, o, w, tm, act, r, t, ws, win_bits);
            if (t) {                                // the learner's outcome, restart (as ttt_step_single_kernel)
                dn = 1;
                wout = ws;
                rew = ws < 0 ? 0 : (ws == s ? 1 : -1);
#pragma unroll
                for (int p = 0; p < P; ++p) o[p] = 0;
                w = -1; tm = 0;
            }
        }
        uint32_t all = 0;
#pragma unroll
        for (int p = 0; p < P; ++p) { occ[p * B + b] = o[p]; all |= o[p]; }
        winner[b] = (int8_t)w;
        to_move[b] = (int8_t)tm;
        tcount[b] = c;
        reward[b] = (int8_t)rew;
        done[b] = (uint8_t)dn;
        winners[b] = (int8_t)wout;
        valid[b] = dd.full & ~all;
    }
#pragma unroll
    for (int p = 0; p < P; ++p) s_occ[p][threadIdx.x] = o[p];
    s_seat[threadIdx.x] = s;
    __syncthreads();
    ttt_write_boards<P>(s_occ, s_seat, dd.n_cells, inv_cells, rel_mod, g0, B, obs);
}

// the outcomes of one wave of playouts into their rows, ttt_playout_kernel's last paragraph word for word (as a function
// of its own: called from there it cost the <8, 4, table> instance a register): lane `lane` played (play) playout r of
// `row`, won by wn (-1: nobody) in len plies
template <int P>
__device__ __forceinline__ void ttt_playout_reduce(const bool live, const uint32_t lane, const uint32_t r, const int R, const uint64_t row,
                                                   const bool play, const int wn, const int len, uint32_t *__restrict__ wins,
                                                   uint32_t *__restrict__ played, uint32_t *__restrict__ len_sum)
{
    // ---- per row segment of this wave: the lanes from a head (r == 0, or lane 0) to the next head
    const unsigned long long heads = __ballot(live && (lane == 0u || r == 0u));
    const unsigned long long above = lane == 63u ? 0ull : heads & (~0ull << (lane + 1u));
    const uint32_t end = above ? (uint32_t)__builtin_ctzll(above) : 64u;
    const unsigned long long seg = (end == 64u ? ~0ull : ((1ull << end) - 1ull)) & (~0ull << lane);
    const bool head = (heads >> lane) & 1ull;
    const bool whole = r == 0u && end - lane == (uint32_t)R;           // the row has no lane in another wave
    uint32_t cnt[P], n_played, plies = 0;
#pragma unroll
    for (int p = 0; p < P; ++p) cnt[p] = (uint32_t)__builtin_popcountll(__ballot(play && wn == p) & seg);
    n_played = (uint32_t)__builtin_popcountll(__ballot(play) & seg);
#pragma unroll
    for (int k = 0; k < 6; ++k)                              // len <= cells + 1 <= 33 < 2^6
        plies += (uint32_t)__builtin_popcountll(__ballot(play && ((len >> k) & 1)) & seg) << k;
    if (head) {
        if (whole) {
#pragma unroll
            for (int p = 0; p < P; ++p) wins[row * P + p] = cnt[p];
            played[row] = n_played;
            len_sum[row] = plies;
        } else if (n_played) {
#pragma unroll
            for (int p = 0; p < P; ++p)
                if (cnt[p]) atomicAdd(&wins[row * P + p], cnt[p]);
            atomicAdd(&played[row], n_played);
            atomicAdd(&len_sum[row], plies);
        }
    }
}

// batched tactical playouts: ttt_playout_kernel's lanes, rows and reduction; every ply behind the candidate is the
// tactical move under the playout tag, its Philox block kept in registers for the two plies it serves
template <int P, int ND, bool WT>
__global__ void __launch_bounds__(256)
ttt_playout_tactical_kernel(const ttt_dirs dd, const int64_t B, const uint32_t seed_lo, const uint32_t seed_hi,
                            const uint64_t first_env_id, const uint64_t thr, const uint32_t *__restrict__ occ,
                            const int8_t *__restrict__ winner, const int8_t *__restrict__ to_move,
                            const uint32_t *__restrict__ tcount, const int32_t *__restrict__ cand, const int A, const int R,
                            const uint64_t n_lanes, uint32_t *__restrict__ wins, uint32_t *__restrict__ played,
                            uint32_t *__restrict__ len_sum, const uint32_t *__restrict__ win_tab)
{
    __shared__ uint32_t win_bits[WT ? 2048 : 1];
    if (WT) {
        ttt_stage_win_table(win_bits, win_tab);
        __syncthreads();
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t wave0 = (uint64_t)blockIdx.x * 256u + (threadIdx.x & ~63u); wave0 < n_lanes; wave0 += stride) {
        // (b, a, r) of this lane, as ttt_playout_kernel
        const uint64_t row0 = wave0 / (uint32_t)R;
        const uint32_t r0 = (uint32_t)(wave0 - row0 * (uint32_t)R);
        const uint32_t q = (r0 + lane) / (uint32_t)R;
        const uint64_t row = row0 + q;
        const uint32_t r = r0 + lane - q * (uint32_t)R;
        const bool live = wave0 + lane < n_lanes;
        const int64_t b = live ? (int64_t)(row / (uint32_t)A) : 0;
        const uint32_t a = (uint32_t)(row - (uint64_t)b * (uint32_t)A);
        int wn = -1, len = 0;
        bool play = false;
        if (live) {
            uint32_t o[P];
#pragma unroll
            for (int p = 0; p < P; ++p) o[p] = occ[p * B + b];
            const uint32_t all = ttt_union<P>(o);
            int w = winner[b], tm = to_move[b];
            play = w < 0 && all != dd.full && (unsigned)tm < (unsigned)P;   // a position that is over skips every row
            int first = -1;
            if (play && cand != nullptr) {                      // the candidate: an empty cell, else the row is skipped
                first = cand[b * A + a];
                play = first >= 0 && first < dd.n_cells && !((all >> (first & 31)) & 1u);
            }
            if (play) {
                const uint32_t g = (uint32_t)(first_env_id + (uint64_t)b), c2 = (a << 16) | r;
                uint32_t c = tcount ? tcount[b] : 0u;
                philox_out rnd = ttt_tactical_block(g, c, c2, CRL_TAG_TTT_TACTICAL_PLAYOUT, seed_lo, seed_hi);
                int term = 0, rw, ws = -1;
                if (first >= 0) {                               // the candidate ply: no draw
                    ttt_step_core<P, ND, WT>(dd, o, w, tm, first, rw, term, ws, win_bits);
                    len = 1;
                }
                while (!term) {
                    const int act = ttt_tactical_move<P, ND>(dd, o, tm, rnd, c, thr);
                    ttt_step_core<P, ND, WT>(dd, o, w, tm, act, rw, term, ws, win_bits);
                    len += 1;
                    c += 1u;
                    if ((c & 1u) == 0u && !term) rnd = ttt_tactical_block(g, c, c2, CRL_TAG_TTT_TACTICAL_PLAYOUT, seed_lo, seed_hi);
                }
                wn = ws;
            }
        }
        ttt_playout_reduce<P>(live, lane, r, R, row, play, wn, len, wins, played, len_sum);
    }
}

// ---- batched Monte Carlo tree search (crl_ttt_mcts; the contract is in include/colosseum_hip.h).  One wave per tree, the
// tree in LDS: n[S + 1] and w[S + 1] as dwords, then the child slots as uint16 [S + 1][cells] with 0 = none (the root is
// nobody's child) -- (S + 1) (8 + 2 cells) bytes, which is what bounds S.  A node's slots are cleared when it is made, so
// nothing but the root is initialised up front.  The descent is wave-uniform: the position is P words every lane holds
// alike, the branches are on ballots and on v_readlane results.  While the wave selects, lane e is cell e; while it
// evaluates, lane r is playout r; while it backs up, lane i is entry i of the path.  The lanes hand values to each other
// through LDS only across ttt_wave_sync (a compiler fence; the LDS itself executes a wave's accesses in order).

__device__ __forceinline__ void ttt_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the maximum of v over the 64 lanes, in every lane: a running maximum inside each row of 16 lanes by DPP row shifts, the
// rows joined by the two row broadcasts, lane 63 read back.  A lane without a source (or outside the row mask) sees 0.
// Every lane of the wave must run it (no lane may sit out a divergent branch around the call).
__device__ __forceinline__ uint32_t ttt_wave_max(uint32_t v)
{
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false));   // row_shr:1
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false));   // row_shr:2
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false));   // row_shr:4
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false));   // row_shr:8
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));   // row_bcast:15 -> rows 1, 3
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));   // row_bcast:31 -> rows 2, 3
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// a wave-uniform word in a vector register: the descent keeps its copy of the position there, alike in every lane, so
// that its plies run on the vector unit beside the playouts' and leave the scalar registers to the kernel's arguments
// (with the position and the line test's temporaries in scalar registers the 13-direction instances spilled them)
__device__ __forceinline__ uint32_t ttt_in_vgpr(const uint32_t x)
{
    uint32_t v;
    asm("v_mov_b32 %0, %1" : "=v"(v) : "s"(x));
    return v;
}

template <class T>
__device__ __forceinline__ T *ttt_in_vgpr(T *const p)
{
    const uint64_t v = (uint64_t)p;
    return (T *)((uint64_t)ttt_in_vgpr((uint32_t)v) | ((uint64_t)ttt_in_vgpr((uint32_t)(v >> 32)) << 32));
}

// floor(num / den) for num < 2^52 and 1 <= den < 2^32: the double quotient is within one of it, the remainder decides
// (the generic 64-bit division is a loop of some hundred instructions, and a selection makes two per cell)
__device__ __forceinline__ uint64_t ttt_mcts_div(const uint64_t num, const uint32_t den)
{
    uint64_t q = (uint64_t)((double)num / (double)den);
    const int64_t r = (int64_t)(num - q * (uint64_t)den);
    q = r < 0 ? q - 1u : (r >= (int64_t)den ? q + 1u : q);
    return q;
}

// the exact floor square root of x < 2^52
__device__ __forceinline__ uint64_t ttt_mcts_isqrt(const uint64_t x)
{
    uint64_t s = (uint64_t)sqrt((double)x);
    s = s * s > x ? s - 1u : ((s + 1u) * (s + 1u) <= x ? s + 1u : s);
    return s;
}

// the contract's piecewise-linear log2 with 8 fraction bits, n >= 1
__device__ __forceinline__ uint32_t ttt_mcts_lg(const uint32_t n)
{
    const uint32_t m = 31u - (uint32_t)__clz((int)n);
    return 256u * m + (((n << (31u - m)) >> 23) & 255u);
}

// LDS, in dwords: [the win-mask table, 2048, if WT][the rank table, 512, if use_rank][a tree of tree_words per wave]
template <int P, int ND, bool WT>
__global__ void __launch_bounds__(256)
ttt_mcts_kernel(const ttt_dirs dd_arg, const int64_t B, const uint32_t seed_lo, const uint32_t seed_hi, const uint64_t first_env_id,
                const uint32_t *occ_arg, const int8_t *winner_arg, const int8_t *to_move_arg, const uint32_t *tcount_arg,
                const int S, const int R, const uint32_t cexp, const uint32_t tree_words, const int use_rank,
                uint32_t *visits_arg, uint32_t *value_arg, uint32_t *nodes_arg, int32_t *best_arg,
                const uint32_t *__restrict__ win_tab)
{
    // What the loops branch on stays in scalar registers; the eight pointers (read or written once per position) and the
    // strides and start masks of the line test move into vector registers, alike in every lane: left where the arguments
    // arrive, these 16 + 2 ND words are live through every loop and the compiler spilled scalar registers around them.
    const uint32_t *occ = ttt_in_vgpr(occ_arg), *tcount = ttt_in_vgpr(tcount_arg);
    const int8_t *winner = ttt_in_vgpr(winner_arg), *to_move = ttt_in_vgpr(to_move_arg);
    uint32_t *visits = ttt_in_vgpr(visits_arg), *value = ttt_in_vgpr(value_arg), *nodes = ttt_in_vgpr(nodes_arg);
    int32_t *best = ttt_in_vgpr(best_arg);
    const bool has_tcount = tcount_arg != nullptr;
    ttt_dirs dd = dd_arg;
    if (!WT) {
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            dd.stride[d] = (int32_t)ttt_in_vgpr((uint32_t)dd_arg.stride[d]);
            dd.start[d] = ttt_in_vgpr(dd_arg.start[d]);
        }
    }
    extern __shared__ __attribute__((aligned(16))) uint32_t mcts_lds[];
    uint32_t *win_bits = mcts_lds;
    uint32_t *rank_words = mcts_lds + (WT ? 2048 : 0);
    const uint8_t (&rank_tab)[256 * 8] = *reinterpret_cast<const uint8_t (*)[256 * 8]>(rank_words);
    uint32_t *trees = rank_words + (use_rank ? 512 : 0);
    if (WT) {
        for (uint32_t i = threadIdx.x; i < 512u; i += blockDim.x)
            reinterpret_cast<uint4 *>(win_bits)[i] = reinterpret_cast<const uint4 *>(win_tab)[i];
    }
    if (use_rank) {                                              // ttt_fill_rank_table, for a workgroup of any size
        for (uint32_t t = threadIdx.x; t < 256u; t += blockDim.x) reinterpret_cast<uint2 *>(rank_words)[t] = ttt_rank_row(t);
    }
    __syncthreads();
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), n_waves = (int)(blockDim.x >> 6);
    const int cells = dd.n_cells;
    uint32_t *n_arr = trees + (uint32_t)wave * tree_words, *w_arr = n_arr + (S + 1);
    uint16_t *child = reinterpret_cast<uint16_t *>(w_arr + (S + 1));
    const bool cell_lane = lane < cells;
    for (int64_t b = (int64_t)blockIdx.x * n_waves + wave; b < B; b += (int64_t)gridDim.x * n_waves) {
        uint32_t o0[P];                                          // (the same words in every lane)
#pragma unroll
        for (int p = 0; p < P; ++p) o0[p] = ttt_in_vgpr((uint32_t)__builtin_amdgcn_readfirstlane((int)occ[p * B + b]));
        const int w0 = __builtin_amdgcn_readfirstlane((int)winner[b]), tm0 = __builtin_amdgcn_readfirstlane((int)to_move[b]);
        const uint32_t tc = has_tcount ? (uint32_t)__builtin_amdgcn_readfirstlane((int)tcount[b]) : 0u;
        const uint32_t g = (uint32_t)(first_env_id + (uint64_t)b);
        if (w0 >= 0 || ttt_union<P>(o0) == dd.full || (unsigned)tm0 >= (unsigned)P) {   // a skipped position: zeros
            if (cell_lane) { visits[b * cells + lane] = 0u; value[b * cells + lane] = 0u; }
            if (lane == 0) { nodes[b] = 0u; best[b] = -1; }
            continue;
        }
        if (lane == 0) { n_arr[0] = 0u; w_arr[0] = 0u; }
        if (cell_lane) child[lane] = 0;
        ttt_wave_sync();
        int nn = 1;                                              // nodes so far
        for (int s = 0; s < S; ++s) {
            uint32_t o[P];
#pragma unroll
            for (int p = 0; p < P; ++p) o[p] = o0[p];
            int w = -1, tm = (int)ttt_in_vgpr((uint32_t)tm0), v = 0, d = 0, term = 0, ws = -1, rw;   // (the mover: with the position)
            uint32_t path = 0;                                   // lane i: the node at depth i of this simulation's path
            for (;;) {
                const uint32_t E = dd.full & ~ttt_union<P>(o);
                const bool in_e = lane < 32 && ((E >> (lane & 31)) & 1u);
                CRL_BOUNDS_LT(in_e ? v * cells + lane : 0, (S + 1) * cells, 210);
                const uint32_t cu = in_e ? child[v * cells + lane] : 0u;
                CRL_BOUNDS_LT(cu, S + 1, 211);
                const unsigned long long fresh = __ballot(in_e && cu == 0u);
                int e, u;
                if (fresh) {                                     // expand: the lowest cell without a child
                    e = (int)__builtin_ctzll(fresh);
                    u = nn++;
                    CRL_BOUNDS_LT(u, S + 1, 212);
                    if (lane == e) child[v * cells + e] = (uint16_t)u;
                    if (cell_lane) child[u * cells + lane] = 0;
                    if (lane == 0) { n_arr[u] = 0u; w_arr[u] = 0u; }
                } else {                                         // select: lane e scores the child at cell e
                    const uint32_t lgv = ttt_mcts_lg(n_arr[v]);
                    uint32_t key = 0;
                    if (in_e) {
                        const uint32_t nu = n_arr[cu], wu = w_arr[cu];
                        const uint64_t exploit = ttt_mcts_div((uint64_t)wu << 15, nu * (uint32_t)R);
                        const uint64_t X = ttt_mcts_div((uint64_t)lgv << 24, nu);
                        const uint64_t score = exploit + (((uint64_t)cexp * ttt_mcts_isqrt(X)) >> 8);   // < 2^26
                        key = (((uint32_t)score << 5) | (uint32_t)(31 - lane)) + 1u;     // ties: the lowest cell
                    }
                    const uint32_t top = ttt_wave_max(key);      // (all lanes: outside the branch above)
                    e = 31 - (int)((top - 1u) & 31u);
                    u = __builtin_amdgcn_readlane((int)cu, e);
                }
                d += 1;
                path = lane == d ? (uint32_t)u : path;
                ttt_step_core<P, ND, WT>(dd, o, w, tm, e, rw, term, ws, win_bits);
                term = __builtin_amdgcn_readfirstlane(term);     // (every lane played the same ply)
                ws = __builtin_amdgcn_readfirstlane(ws);
                if (fresh || term || d >= 32) break;             // (d >= 32: never, a ply that fills the board is terminal)
                v = u;
            }
            // ---- evaluate the leaf: the outcome of the ply into it, or R random playouts, lane r playout r
            uint32_t cnt[P], draws;                              // (wave-uniform sums, kept in vector registers)
#pragma unroll
            for (int p = 0; p < P; ++p) cnt[p] = ttt_in_vgpr(term && ws == p ? (uint32_t)R : 0u);
            draws = ttt_in_vgpr(term && ws < 0 ? (uint32_t)R : 0u);
            if (!term) {
                for (int r0 = 0; r0 < R; r0 += 64) {
                    const uint32_t r = (uint32_t)(r0 + lane);
                    const bool live = r < (uint32_t)R;
                    int wn = -1;
                    if (live) {
                        uint32_t po[P];
#pragma unroll
                        for (int p = 0; p < P; ++p) po[p] = o[p];
                        int pw = w, ptm = tm, pterm = 0, prw, pws = -1;
                        const uint32_t c2 = ((uint32_t)s << 16) | r;
                        uint32_t c = tc + (uint32_t)d;
                        philox_out rnd = philox4x32_10<true>(g, c >> 3, c2, CRL_TAG_TTT_MCTS, seed_lo, seed_hi);
                        for (int left = 33; !pterm && left > 0; --left) {   // ttt_playout_kernel's random ply (left: never runs out)
                            const uint32_t empty = dd.full & ~ttt_union<P>(po);
                            const uint32_t n_empty = (uint32_t)__popc(empty);       // (not 0: the game is running)
                            const uint32_t sel = (c >> 1) & 3u;
                            uint32_t word = rnd.w[0];
                            word = (sel == 1) ? rnd.w[1] : word;
                            word = (sel == 2) ? rnd.w[2] : word;
                            word = (sel == 3) ? rnd.w[3] : word;
                            word = (c & 1u) ? word * (n_empty + 1u) : word;
                            const uint32_t rank = __umulhi(word, n_empty);
                            const int act = use_rank ? (int)nth_set_bit_tab<WT>(rank_tab, empty, rank) : nth_set_bit(empty, (int)rank);
                            ttt_step_core<P, ND, WT>(dd, po, pw, ptm, act, prw, pterm, pws, win_bits);
                            c += 1u;
                            if ((c & 7u) == 0u && !pterm) rnd = philox4x32_10<true>(g, c >> 3, c2, CRL_TAG_TTT_MCTS, seed_lo, seed_hi);
                        }
                        wn = pws;
                    }
#pragma unroll
                    for (int p = 0; p < P; ++p) cnt[p] += ttt_in_vgpr((uint32_t)__builtin_popcountll(__ballot(live && wn == p)));
                    draws += ttt_in_vgpr((uint32_t)__builtin_popcountll(__ballot(live && wn < 0)));
                }
            }
            // ---- back up: lane i adds to the node at depth i (distinct nodes: no atomics), q = who moved into it
            ttt_wave_sync();
            if (lane <= d) {
                uint32_t add = 0;
                if (lane > 0) {
                    const int q = (tm0 + lane - 1) % P;
                    uint32_t mine = 0;
#pragma unroll
                    for (int p = 0; p < P; ++p) mine = (p == q) ? cnt[p] : mine;
                    add = 2u * mine + draws;
                }
                CRL_BOUNDS_LT(path, S + 1, 213);
                n_arr[path] += 1u;
                w_arr[path] += add;
            }
            ttt_wave_sync();
        }
        // ---- the root's children: visits, value, the most visited (then the larger w, then the lowest cell)
        const uint32_t cu = cell_lane ? child[lane] : 0u;
        const uint32_t vis = cu ? n_arr[cu] : 0u, val = cu ? w_arr[cu] : 0u;
        if (cell_lane) { visits[b * cells + lane] = vis; value[b * cells + lane] = val; }
        const uint32_t top_n = ttt_wave_max(vis);                // (a child has n >= 1)
        const bool most = cu != 0u && vis == top_n;
        const uint32_t top_w = ttt_wave_max(most ? val + 1u : 0u);
        const unsigned long long pick = __ballot(most && val + 1u == top_w);
        if (lane == 0) { nodes[b] = (uint32_t)nn; best[b] = pick ? (int32_t)__builtin_ctzll(pick) : -1; }
        ttt_wave_sync();                                         // the next tree starts behind these reads
    }
}

// ---- the search as a seated agent (crl_ttt_sample_mcts / _rollout_mcts / _step_single_mcts; the contract is in
// include/colosseum_hip.h).  One wave per game and ttt_mcts_kernel's LDS layout; outside the search the wave holds the
// game's position as P words every lane holds alike, and what it branches on goes through v_readfirstlane.
//
// One search of the running position (o0, mover tm0) at step counter tc of game g, winner taken as -1: the root's most
// visited cell (ties: the larger w, then the lowest cell).  The text is ttt_mcts_kernel's tree loop and root scan, side by
// side with it: that kernel's instances keep their registers this way.  Every lane of the wave must call it.
template <int P, int ND, bool WT>
__device__ __forceinline__ int ttt_search_best(const ttt_dirs &dd, const uint32_t (&o0)[P], const int tm0, const uint32_t tc, const uint32_t g,
                                               const uint32_t seed_lo, const uint32_t seed_hi, const int S, const int R, const uint32_t cexp,
                                               const int use_rank, const uint32_t *win_bits, const uint8_t (&rank_tab)[256 * 8],
                                               uint32_t *n_arr, uint32_t *w_arr, uint16_t *child, const int lane)
{
    const int cells = dd.n_cells;
    const bool cell_lane = lane < cells;
    if (lane == 0) { n_arr[0] = 0u; w_arr[0] = 0u; }
    if (cell_lane) child[lane] = 0;
    ttt_wave_sync();
    int nn = 1;                                                  // nodes so far
    for (int s = 0; s < S; ++s) {
        uint32_t o[P];
#pragma unroll
        for (int p = 0; p < P; ++p) o[p] = o0[p];
        int w = -1, tm = (int)ttt_in_vgpr((uint32_t)tm0), v = 0, d = 0, term = 0, ws = -1, rw;
        uint32_t path = 0;                                       // lane i: the node at depth i of this simulation's path
        for (;;) {
            const uint32_t E = dd.full & ~ttt_union<P>(o);
            const bool in_e = lane < 32 && ((E >> (lane & 31)) & 1u);
            CRL_BOUNDS_LT(in_e ? v * cells + lane : 0, (S + 1) * cells, 220);
            const uint32_t cu = in_e ? child[v * cells + lane] : 0u;
            CRL_BOUNDS_LT(cu, S + 1, 221);
            const unsigned long long fresh = __ballot(in_e && cu == 0u);
            int e, u;
            if (fresh) {                                         // expand: the lowest cell without a child
                e = (int)__builtin_ctzll(fresh);
                u = nn++;
                CRL_BOUNDS_LT(u, S + 1, 222);
                if (lane == e) child[v * cells + e] = (uint16_t)u;
                if (cell_lane) child[u * cells + lane] = 0;
                if (lane == 0) { n_arr[u] = 0u; w_arr[u] = 0u; }
            } else {                                             // select: lane e scores the child at cell e
                const uint32_t lgv = ttt_mcts_lg(n_arr[v]);
                uint32_t key = 0;
                if (in_e) {
                    const uint32_t nu = n_arr[cu], wu = w_arr[cu];
                    const uint64_t exploit = ttt_mcts_div((uint64_t)wu << 15, nu * (uint32_t)R);
                    const uint64_t X = ttt_mcts_div((uint64_t)lgv << 24, nu);
                    const uint64_t score = exploit + (((uint64_t)cexp * ttt_mcts_isqrt(X)) >> 8);   // < 2^26
                    key = (((uint32_t)score << 5) | (uint32_t)(31 - lane)) + 1u;     // ties: the lowest cell
                }
                const uint32_t top = ttt_wave_max(key);          // (all lanes: outside the branch above)
                e = 31 - (int)((top - 1u) & 31u);
                u = __builtin_amdgcn_readlane((int)cu, e);
            }
            d += 1;
            path = lane == d ? (uint32_t)u : path;
            ttt_step_core<P, ND, WT>(dd, o, w, tm, e, rw, term, ws, win_bits);
            term = __builtin_amdgcn_readfirstlane(term);         // (every lane played the same ply)
            ws = __builtin_amdgcn_readfirstlane(ws);
            if (fresh || term || d >= 32) break;                 // (d >= 32: never, a ply that fills the board is terminal)
            v = u;
        }
        // ---- evaluate the leaf: the outcome of the ply into it, or R random playouts, lane r playout r
        uint32_t cnt[P], draws;                                  // (wave-uniform sums, kept in vector registers)
#pragma unroll
        for (int p = 0; p < P; ++p) cnt[p] = ttt_in_vgpr(term && ws == p ? (uint32_t)R : 0u);
        draws = ttt_in_vgpr(term && ws < 0 ? (uint32_t)R : 0u);
        if (!term) {
            for (int r0 = 0; r0 < R; r0 += 64) {
                const uint32_t r = (uint32_t)(r0 + lane);
                const bool live = r < (uint32_t)R;
                int wn = -1;
                if (live) {
                    uint32_t po[P];
#pragma unroll
                    for (int p = 0; p < P; ++p) po[p] = o[p];
                    int pw = w, ptm = tm, pterm = 0, prw, pws = -1;
                    const uint32_t c2 = ((uint32_t)s << 16) | r;
                    uint32_t c = tc + (uint32_t)d;
                    philox_out rnd = philox4x32_10<true>(g, c >> 3, c2, CRL_TAG_TTT_MCTS, seed_lo, seed_hi);
                    for (int left = 33; !pterm && left > 0; --left) {   // ttt_playout_kernel's random ply (left: never runs out)
                        const uint32_t empty = dd.full & ~ttt_union<P>(po);
                        const uint32_t n_empty = (uint32_t)__popc(empty);       // (not 0: the game is running)
                        const uint32_t sel = (c >> 1) & 3u;
                        uint32_t word = rnd.w[0];
                        word = (sel == 1) ? rnd.w[1] : word;
                        word = (sel == 2) ? rnd.w[2] : word;
                        word = (sel == 3) ? rnd.w[3] : word;
                        word = (c & 1u) ? word * (n_empty + 1u) : word;
                        const uint32_t rank = __umulhi(word, n_empty);
                        const int act = use_rank ? (int)nth_set_bit_tab<WT>(rank_tab, empty, rank) : nth_set_bit(empty, (int)rank);
                        ttt_step_core<P, ND, WT>(dd, po, pw, ptm, act, prw, pterm, pws, win_bits);
                        c += 1u;
                        if ((c & 7u) == 0u && !pterm) rnd = philox4x32_10<true>(g, c >> 3, c2, CRL_TAG_TTT_MCTS, seed_lo, seed_hi);
                    }
                    wn = pws;
                }
#pragma unroll
                for (int p = 0; p < P; ++p) cnt[p] += ttt_in_vgpr((uint32_t)__builtin_popcountll(__ballot(live && wn == p)));
                draws += ttt_in_vgpr((uint32_t)__builtin_popcountll(__ballot(live && wn < 0)));
            }
        }
        // ---- back up: lane i adds to the node at depth i (distinct nodes: no atomics), q = who moved into it
        ttt_wave_sync();
        if (lane <= d) {
            uint32_t add = 0;
            if (lane > 0) {
                const int q = (tm0 + lane - 1) % P;
                uint32_t mine = 0;
#pragma unroll
                for (int p = 0; p < P; ++p) mine = (p == q) ? cnt[p] : mine;
                add = 2u * mine + draws;
            }
            CRL_BOUNDS_LT(path, S + 1, 223);
            n_arr[path] += 1u;
            w_arr[path] += add;
        }
        ttt_wave_sync();
    }
    // ---- the root's most visited child (then the larger w, then the lowest cell)
    const uint32_t cu = cell_lane ? child[lane] : 0u;
    CRL_BOUNDS_LT(cu, S + 1, 224);
    const uint32_t vis = cu ? n_arr[cu] : 0u, val = cu ? w_arr[cu] : 0u;
    const uint32_t top_n = ttt_wave_max(vis);                    // (a child has n >= 1)
    const bool most = cu != 0u && vis == top_n;
    const uint32_t top_w = ttt_wave_max(most ? val + 1u : 0u);
    const unsigned long long pick = __ballot(most && val + 1u == top_w);
    ttt_wave_sync();                                             // the next tree starts behind these reads
    return pick ? (int)__builtin_ctzll(pick) : -1;
}

// the three frames around the agent's move, one kernel text: which one is a template parameter
enum { TTT_FRAME_SAMPLE = 0, TTT_FRAME_ROLLOUT = 1, TTT_FRAME_SINGLE = 2 };

// what the frames read and write besides the state (each frame its own part; the rest is NULL / 0)
struct ttt_agent_io {
    uint32_t *tcount;                                            // sample, step_single (the rollout's is st.tcount)
    int8_t *action;                                              // sample
    int advance;
    int T;                                                       // rollout
    crl_ttt_stats st;
    const int8_t *seat;                                          // step_single
    const int64_t *learner_action;
    int8_t *reward;
    uint8_t *done;
    int8_t *winners, *obs;
    uint32_t *valid;
    int rel_mod;
};

// LDS as ttt_mcts_kernel: [the win-mask table, 2048, if WT][the rank table, 512, if use_rank][a tree of tree_words per wave]
template <int P, int ND, bool WT, int FRAME>
__global__ void __launch_bounds__(256)
ttt_mcts_agent_kernel(const ttt_dirs dd_arg, const int64_t B, const uint32_t seed_lo, const uint32_t seed_hi, const uint64_t first_env_id,
                      const uint64_t thr, const int S, const int R, const uint32_t cexp, const uint32_t tree_words, const int use_rank,
                      uint32_t *occ_arg, int8_t *winner_arg, int8_t *to_move_arg, const ttt_agent_io io,
                      const uint32_t *__restrict__ win_tab)
{
    // (the pointers and the line test's strides and start masks in vector registers, as ttt_mcts_kernel has them)
    uint32_t *occ = ttt_in_vgpr(occ_arg);
    int8_t *winner = ttt_in_vgpr(winner_arg), *to_move = ttt_in_vgpr(to_move_arg);
    ttt_dirs dd = dd_arg;
    if (!WT) {
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            dd.stride[d] = (int32_t)ttt_in_vgpr((uint32_t)dd_arg.stride[d]);
            dd.start[d] = ttt_in_vgpr(dd_arg.start[d]);
        }
    }
    extern __shared__ __attribute__((aligned(16))) uint32_t mcts_lds[];
    uint32_t *win_bits = mcts_lds;
    uint32_t *rank_words = mcts_lds + (WT ? 2048 : 0);
    const uint8_t (&rank_tab)[256 * 8] = *reinterpret_cast<const uint8_t (*)[256 * 8]>(rank_words);
    uint32_t *trees = rank_words + (use_rank ? 512 : 0);
    if (WT) {
        for (uint32_t i = threadIdx.x; i < 512u; i += blockDim.x)
            reinterpret_cast<uint4 *>(win_bits)[i] = reinterpret_cast<const uint4 *>(win_tab)[i];
    }
    if (use_rank) {
        for (uint32_t t = threadIdx.x; t < 256u; t += blockDim.x) reinterpret_cast<uint2 *>(rank_words)[t] = ttt_rank_row(t);
    }
    __syncthreads();
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), n_waves = (int)(blockDim.x >> 6);
    const int cells = dd.n_cells;
    uint32_t *n_arr = trees + (uint32_t)wave * tree_words, *w_arr = n_arr + (S + 1);
    uint16_t *child = reinterpret_cast<uint16_t *>(w_arr + (S + 1));
    // the agent's move for the mover tm on the position o at step counter c of game g (rules 1 to 5 of the contract)
    auto agent_move = [&](const uint32_t (&o)[P], const int tm, const uint32_t c, const uint32_t g) -> int {
        const uint32_t E = (uint32_t)__builtin_amdgcn_readfirstlane((int)(dd.full & ~ttt_union<P>(o)));
        if ((unsigned)tm >= (unsigned)P || E == 0u) return -1;
        const philox_out rnd = ttt_tactical_block(g, c, 0u, CRL_TAG_TTT_TACTICAL, seed_lo, seed_hi);
        const uint32_t u = (uint32_t)__builtin_amdgcn_readfirstlane((int)((c & 1u) ? rnd.w[2] : rnd.w[0]));
        if ((uint64_t)u < thr) {                                 // a noisy ply: a uniform empty cell, no search
            const uint32_t v = (c & 1u) ? rnd.w[3] : rnd.w[1];
            return __builtin_amdgcn_readfirstlane(nth_set_bit(E, (int)__umulhi(v, (uint32_t)__popc(E))));
        }
        return ttt_search_best<P, ND, WT>(dd, o, tm, c, g, seed_lo, seed_hi, S, R, cexp, use_rank, win_bits, rank_tab, n_arr, w_arr,
                                          child, lane);
    };
    // a ply of the wave's game, every lane alike: what the frames branch on comes back wave-uniform
    auto play = [&](uint32_t (&o)[P], int &w, int &tm, const int action, int &term, int &ws) {
        int r;
        ttt_step_core<P, ND, WT>(dd, o, w, tm, action, r, term, ws, win_bits);
        w = __builtin_amdgcn_readfirstlane(w);
        tm = __builtin_amdgcn_readfirstlane(tm);
        term = __builtin_amdgcn_readfirstlane(term);
        ws = __builtin_amdgcn_readfirstlane(ws);
    };
    for (int64_t b = (int64_t)blockIdx.x * n_waves + wave; b < B; b += (int64_t)gridDim.x * n_waves) {
        uint32_t o[P];                                           // (the same words in every lane)
#pragma unroll
        for (int p = 0; p < P; ++p) o[p] = ttt_in_vgpr((uint32_t)__builtin_amdgcn_readfirstlane((int)occ[p * B + b]));
        int tm = __builtin_amdgcn_readfirstlane((int)to_move[b]);
        const uint32_t g = (uint32_t)(first_env_id + (uint64_t)b);
        if constexpr (FRAME == TTT_FRAME_SAMPLE) {
            uint32_t *tcount = ttt_in_vgpr(io.tcount);
            const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane((int)tcount[b]);
            const int act = agent_move(o, tm, c, g);
            if (lane == 0) {
                ttt_in_vgpr(io.action)[b] = (int8_t)act;
                if (io.advance) tcount[b] = c + 1u;
            }
        } else if constexpr (FRAME == TTT_FRAME_ROLLOUT) {
            // crl_ttt_rollout_tactical's ply (ttt_step_core, the restart, the statistics) with the search agent's move; position,
            // counters and statistics stay in registers over the T plies
            const crl_ttt_stats &st = io.st;
            int w = __builtin_amdgcn_readfirstlane((int)winner[b]);
            uint32_t tc = (uint32_t)__builtin_amdgcn_readfirstlane((int)st.tcount[b]);
            uint32_t ts = (uint32_t)__builtin_amdgcn_readfirstlane((int)st.tstep[b]), n_ep = 0, draws = 0, len_sum = 0, wins[P];
#pragma unroll
            for (int p = 0; p < P; ++p) wins[p] = 0;
            for (int t = 0; t < io.T; ++t) {
                const int action = agent_move(o, tm, tc, g);
                int term, ws;
                play(o, w, tm, action, term, ws);
                ts += 1;
                tc += 1;
                if (term) {
                    n_ep += 1;
                    len_sum += ts;
                    draws += (ws < 0);
#pragma unroll
                    for (int p = 0; p < P; ++p) { wins[p] += (ws == p); o[p] = 0; }
                    w = -1; tm = 0; ts = 0;
                }
            }
            if (lane == 0) {
                int32_t *row = st.results ? st.results + b * (3 + P) : nullptr;    // packed result row, as crl_ttt_rollout writes it
#pragma unroll
                for (int p = 0; p < P; ++p) {
                    occ[p * B + b] = o[p];
                    const uint32_t wc = st.win_count[p * B + b] + wins[p];
                    st.win_count[p * B + b] = wc;
                    if (row) row[3 + p] = (int32_t)wc;
                }
                winner[b] = (int8_t)w;
                to_move[b] = (int8_t)tm;
                st.tcount[b] = tc;
                st.tstep[b] = ts;
                const uint32_t ne = st.n_episodes[b] + n_ep, dr = st.draw_count[b] + draws, ls = st.len_sum[b] + len_sum;
                st.n_episodes[b] = ne;
                st.draw_count[b] = dr;
                st.len_sum[b] = ls;
                if (row) { row[0] = (int32_t)ne; row[1] = (int32_t)ls; row[2] = (int32_t)dr; }
            }
        } else {
            // ttt_step_single_kernel's loop, wave-uniform, with the opponents' plies from the search agent
            uint32_t *tcount = ttt_in_vgpr(io.tcount);
            int w = __builtin_amdgcn_readfirstlane((int)winner[b]);
            int s = (int)io.seat[b] % P;
            s += s < 0 ? P : 0;
            s = __builtin_amdgcn_readfirstlane(s);
            uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane((int)tcount[b]);
            int rew = 0, dn = 0, wout = -1;
            bool learner = io.learner_action != nullptr && tm == s;
            for (int opp = 0; learner || (tm != s && opp < 2 * (P - 1)); ) {
                int act;
                if (learner) {                          // crl_ttt_step's int8 action for v in [-1, cells), else the pass
                    const int64_t v = io.learner_action[b];
                    act = __builtin_amdgcn_readfirstlane((v >= -1 && v < cells) ? (int)v : -1);
                } else {                                // crl_ttt_sample_mcts at this game's step counter
                    act = agent_move(o, tm, c, g);
                    ++opp;
                }
                c += 1u;
                learner = false;
                int t, ws;
                play(o, w, tm, act, t, ws);
                if (t) {                                // the learner's outcome, restart (as ttt_step_single_kernel)
                    dn = 1;
                    wout = ws;
                    rew = ws < 0 ? 0 : (ws == s ? 1 : -1);
#pragma unroll
                    for (int p = 0; p < P; ++p) o[p] = 0;
                    w = -1; tm = 0;
                }
            }
            if (lane == 0) {
#pragma unroll
                for (int p = 0; p < P; ++p) occ[p * B + b] = o[p];
                winner[b] = (int8_t)w;
                to_move[b] = (int8_t)tm;
                tcount[b] = c;
                io.reward[b] = (int8_t)rew;
                io.done[b] = (uint8_t)dn;
                io.winners[b] = (int8_t)wout;
                io.valid[b] = dd.full & ~ttt_union<P>(o);
            }
            if (lane < cells) {                          // the learner's observation, lane = cell (ttt_write_boards' rule)
                int v = -1;
#pragma unroll
                for (int p = 0; p < P; ++p) v = ((o[p] >> lane) & 1u) ? p : v;
                if (v >= 0) {
                    const int rr = (v - s) % io.rel_mod;
                    v = rr < 0 ? rr + io.rel_mod : rr;
                }
                io.obs[b * cells + lane] = (int8_t)v;
            }
        }
    }
}

__global__ void __launch_bounds__(256)
ttt_reset_kernel(const int P, const int64_t B, const uint8_t *__restrict__ mask, uint32_t *__restrict__ occ,
                 int8_t *__restrict__ winner, int8_t *__restrict__ to_move)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if (mask && !mask[b]) return;
    for (int p = 0; p < P; ++p) occ[p * B + b] = 0;
    winner[b] = -1;
    to_move[b] = 0;
}

__global__ void __launch_bounds__(256)
ttt_valid_kernel(const int P, const uint32_t full, const int64_t B, const uint32_t *__restrict__ occ, uint32_t *__restrict__ valid)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    uint32_t all = 0;
    for (int p = 0; p < P; ++p) all |= occ[p * B + b];
    valid[b] = full & ~all;
}

// board export / state_to_observation for 256 games per workgroup: masks into LDS (coalesced), then ttt_write_boards
template <int P>
__global__ void __launch_bounds__(256)
ttt_board_kernel(const int n_cells, const uint32_t inv_cells, const int64_t B, const uint32_t *__restrict__ occ,
                 const int8_t *__restrict__ player, const int rel_mod, int8_t *__restrict__ board)
{
    __shared__ uint32_t s_occ[P][256];
    __shared__ int s_rel[256];
    const int64_t g0 = (int64_t)blockIdx.x * 256;
    const int64_t b = g0 + threadIdx.x;
#pragma unroll
    for (int p = 0; p < P; ++p) s_occ[p][threadIdx.x] = b < B ? occ[p * B + b] : 0u;
    s_rel[threadIdx.x] = (player && b < B) ? (int)player[b] : -1;
    __syncthreads();
    ttt_write_boards<P>(s_occ, s_rel, n_cells, inv_cells, rel_mod, g0, B, board);
}

// ---- the same calls on states in the REFERENCE's own layout (tictactoe_2p_env.py:165-169): board int8 [B][cells], -1 =
// empty, else the owner's id.  For callers that hold reference states -- the single-state drop-in classes above all
// (one launch per next_state on host-mapped memory, crl_host_alloc) -- and never see the occupancy masks.  One lane per
// game: it gathers its cells into the per-player masks, plays the very ttt_step_core of crl_ttt_step, and writes back
// what changed.
template <int P>
__device__ __forceinline__ void ttt_masks_of_board(const int8_t *__restrict__ cells, const int n_cells, uint32_t (&o)[P])
{
#pragma unroll
    for (int p = 0; p < P; ++p) o[p] = 0u;
    for (int c = 0; c < n_cells; ++c) {
        const int v = cells[c];
#pragma unroll
        for (int p = 0; p < P; ++p) o[p] |= (v == p) ? (1u << c) : 0u;
    }
}

// observation of one game: ids relative to `rel` (python's non-negative modulo by rel_mod), -1 stays -1
template <int P>
__device__ __forceinline__ void ttt_write_relative(const uint32_t (&o)[P], const int n_cells, const int rel, const int rel_mod,
                                                   int8_t *__restrict__ out)
{
    for (int c = 0; c < n_cells; ++c) {
        int v = -1;
#pragma unroll
        for (int p = 0; p < P; ++p) v = ((o[p] >> c) & 1u) ? p : v;
        if (v >= 0 && rel >= 0) {
            const int rr = (v - rel) % rel_mod;
            v = rr < 0 ? rr + rel_mod : rr;
        }
        out[c] = (int8_t)v;
    }
}

// one reference-layout state BY VALUE (kernel arguments): what the single-state call passes instead of letting the kernel
// fetch board, winner, mover and action over PCIe first (crl_ttt_step_board_host)
struct TttVec {
    uint32_t occ[CRL_TTT_MAX_P];                               // the board as the masks ttt_masks_of_board would build
    int32_t winner, to_move, action;
};

template <int P, int ND>
__global__ void __launch_bounds__(256)
ttt_step_board_kernel(const ttt_dirs dd, const int64_t B, int8_t *__restrict__ board, int8_t *__restrict__ winner,
                      int8_t *__restrict__ to_move, const int8_t *__restrict__ action, int8_t *__restrict__ reward,
                      uint8_t *__restrict__ terminal, int8_t *__restrict__ winners, uint32_t *__restrict__ valid,
                      int8_t *__restrict__ obs, const int rel_mod, const uint32_t flags,
                      const TttVec vec, const bool by_value, uint32_t *flag, const uint32_t seq)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int8_t *cells = board + b * dd.n_cells;
    uint32_t o[P];
    if (by_value) {
#pragma unroll
        for (int p = 0; p < P; ++p) o[p] = vec.occ[p];
    } else {
        ttt_masks_of_board<P>(cells, dd.n_cells, o);
    }
    const uint32_t before = ttt_union<P>(o);
    int w = by_value ? vec.winner : (int)winner[b], tm = by_value ? vec.to_move : (int)to_move[b], r, t, ws;
    const int pl = tm, act = by_value ? vec.action : (int)action[b];
    ttt_step_core<P, ND>(dd, o, w, tm, act, r, t, ws);
    reward[b] = (int8_t)r;
    terminal[b] = (uint8_t)t;
    winners[b] = (int8_t)ws;
    uint32_t all = ttt_union<P>(o);
    if (t && (flags & CRL_STEP_AUTO_RESET)) {
#pragma unroll
        for (int p = 0; p < P; ++p) o[p] = 0;
        all = 0; w = -1; tm = 0;
        for (int c = 0; c < dd.n_cells; ++c) cells[c] = (int8_t)-1;
    } else if (all != before) {
        cells[act] = (int8_t)pl;                   // the one cell the move filled (tictactoe_2p_env.py:295)
    }
    winner[b] = (int8_t)w;
    to_move[b] = (int8_t)tm;
    if (valid) valid[b] = dd.full & ~all;          // valid_actions of the player to move next (:317-348)
    if (obs) ttt_write_relative<P>(o, dd.n_cells, tm, rel_mod, obs + b * dd.n_cells);
    // (single-state call, B = 1: this thread wrote everything, so its release store publishes completion)
    if (flag && b == 0) __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// valid_actions (empties mask) and / or state_to_observation (ids relative to player[b]) of reference-layout boards
template <int P>
__global__ void __launch_bounds__(256)
ttt_observe_board_kernel(const int n_cells, const uint32_t full, const int64_t B, const int8_t *__restrict__ board,
                         const int8_t *__restrict__ player, const int rel_mod, int8_t *__restrict__ obs,
                         uint32_t *__restrict__ valid)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    uint32_t o[P];
    ttt_masks_of_board<P>(board + b * n_cells, n_cells, o);
    if (valid) valid[b] = full & ~ttt_union<P>(o);
    if (obs) ttt_write_relative<P>(o, n_cells, player ? (int)player[b] : -1, rel_mod, obs + b * n_cells);
}

inline unsigned blocks_for(int64_t n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

// host: enumerate directions / lines exactly like the oracle does, independently written
int build_dirs(const crl_ttt_cfg &c, ttt_dirs &dd, uint32_t *lines, int &n_lines)
{
    memset(&dd, 0, sizeof(dd));
    dd.K = c.K; dd.P = c.P; dd.n_cells = c.n_cells; dd.full = c.full;
    n_lines = 0;
    for (int di = 0; di <= 1; ++di)
        for (int dj = -1; dj <= 1; ++dj)
            for (int dk = -1; dk <= 1; ++dk) {
                if (di == 0 && dj < 0) continue;
                if (di == 0 && dj == 0 && dk <= 0) continue;
                const int stride = (di * c.D1 + dj) * c.D2 + dk;
                uint32_t start = 0;
                for (int i = 0; i < c.D0; ++i)
                    for (int j = 0; j < c.D1; ++j)
                        for (int k = 0; k < c.D2; ++k) {
                            const int ei = i + di * (c.K - 1), ej = j + dj * (c.K - 1), ek = k + dk * (c.K - 1);
                            if (ei < 0 || ei >= c.D0 || ej < 0 || ej >= c.D1 || ek < 0 || ek >= c.D2) continue;
                            const int cell = (i * c.D1 + j) * c.D2 + k;
                            start |= 1u << cell;
                            uint32_t m = 0;
                            for (int s = 0; s < c.K; ++s) m |= 1u << (cell + s * stride);
                            if (n_lines >= CRL_TTT_MAX_LINES) return -1;
                            lines[n_lines++] = m;
                        }
                if (start) {
                    if (stride <= 0 || dd.n_dirs >= 13) return -2;
                    dd.stride[dd.n_dirs] = stride;
                    dd.start[dd.n_dirs] = start;
                    dd.n_dirs++;
                }
            }
    return 0;
}

inline const ttt_dirs &dirs_of(const crl_ctx *ctx) { return ctx->ttt_dd; }     // built once, in crl_ttt_create

// the win-mask table of a board of at most 16 cells, if it lives on the current device; else nullptr (there is none, or
// the call runs on another device than crl_ttt_create did): the kernels then compute the line test
inline const uint32_t *ttt_win_table_here(const crl_ctx *ctx)
{
    int dev = -1;
    return ctx->ttt_win_dev && hipGetDevice(&dev) == hipSuccess && dev == ctx->ttt_win_device ? ctx->ttt_win_dev : nullptr;
}

// floor(2^32 / cells) + 1: ttt_write_boards divides by the cell count with one multiply-high
inline uint32_t ttt_inv_cells(const int cells) { return cells == 1 ? 0u : (uint32_t)(((uint64_t)1 << 32) / (uint64_t)cells) + 1u; }

#endif // TTT_DEVICE_ONLY (the kernels)

} // namespace

#define TTT_DISPATCH_P(P_, ...)            \
    switch (P_) {                          \
        case 1: { constexpr int PP = 1; __VA_ARGS__; } break; \
        case 2: { constexpr int PP = 2; __VA_ARGS__; } break; \
        case 3: { constexpr int PP = 3; __VA_ARGS__; } break; \
        case 4: { constexpr int PP = 4; __VA_ARGS__; } break; \
        case 5: { constexpr int PP = 5; __VA_ARGS__; } break; \
        case 6: { constexpr int PP = 6; __VA_ARGS__; } break; \
        case 7: { constexpr int PP = 7; __VA_ARGS__; } break; \
        case 8: { constexpr int PP = 8; __VA_ARGS__; } break; \
        default: crl_set_error("ttt: P=%d out of range 1..8", P_); return CRL_EINVAL; \
    }

// ---- which template instance of a kernel runs a context: the rule is stated here and nowhere else.  The statement(s) given
// see PP = the player count and, with TTT_DISPATCH_ND, NDD = 4 for a board with at most 4 line directions (everything 1-D
// and 2-D), else 13; with TTT_DISPATCH_ND_WT also WTT, the win test out of the table: only with NDD = 4, at most 16 cells
// and the table on this device (win_tab_ = ttt_win_table_here).
#define TTT_INSTANCE(ND_, WT_, ...) { constexpr int NDD = ND_; [[maybe_unused]] constexpr bool WTT = WT_; __VA_ARGS__; }
#define TTT_DISPATCH_ND(ctx_, ...)                                                          \
    TTT_DISPATCH_P((ctx_)->ttt.P, {                                                          \
        if ((ctx_)->ttt_dd.n_dirs <= 4) TTT_INSTANCE(4, false, __VA_ARGS__)                  \
        else TTT_INSTANCE(13, false, __VA_ARGS__)                                            \
    })
#define TTT_DISPATCH_ND_WT(ctx_, win_tab_, ...)                                             \
    TTT_DISPATCH_P((ctx_)->ttt.P, {                                                          \
        if ((ctx_)->ttt_dd.n_dirs > 4) TTT_INSTANCE(13, false, __VA_ARGS__)                  \
        else if ((ctx_)->ttt_dd.n_cells <= 16 && (win_tab_) != nullptr) TTT_INSTANCE(4, true, __VA_ARGS__) \
        else TTT_INSTANCE(4, false, __VA_ARGS__)                                             \
    })
// (every kernel here runs one game -- the playout: one playout -- per thread, 256 to a workgroup, on the caller's `stream`)
#define TTT_LAUNCH(kernel, blocks, ...) hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__)

#define TTT_CTX_CHECK(fn)                                                                  \
    CRL_REQUIRE(ctx != nullptr && ctx->game == CRL_GAME_TTT, "%s: ctx is not a tictactoe context", fn); \
    CRL_REQUIRE(B > 0 && B <= ((int64_t)1 << 31), "%s: B=%lld out of range", fn, (long long)B)
// (a launcher that serves an agent's entry as well gets its noise by pointer, NULL from the random agent's entry, and
// checks it where the tactical entry always did)
#define TTT_NOISE_CHECK(fn) CRL_REQUIRE(noise == nullptr || (*noise >= 0.0 && *noise <= 1.0), "%s: noise=%g outside [0, 1]", fn, *noise)   /* (NaN fails too) */

#ifndef TTT_DEVICE_ONLY

int crl_ttt_bounds(unsigned int *out4)
{
    CRL_BOUNDS_READBACK(out4);
    return CRL_OK;
}

// S_max of crl_ttt_mcts (include/colosseum_hip.h): a tree of S + 1 nodes of 8 + 2 cells bytes within 64 KB, s in 12 bits
static int ttt_mcts_max_simulations(const int cells)
{
    const int s = 65536 / (8 + 2 * cells) - 1;
    return s < 4095 ? s : 4095;
}

// the parameters of a search, crl_ttt_mcts's own or a search agent's (NULL in a launcher that serves the other agents too):
// the limits of include/colosseum_hip.h, stated here and nowhere else
struct ttt_search { int S, R; uint32_t cexp; };
#define TTT_SEARCH_CHECK(fn)                                                                                          \
    if (search) {                                                                                                     \
        const int cells_ = ctx->ttt.n_cells, s_max_ = ttt_mcts_max_simulations(cells_);                               \
        CRL_REQUIRE(search->S >= 1 && search->S <= s_max_, "%s: S=%d out of range 1..%d (a board of %d cells)", fn, search->S, s_max_, cells_); \
        CRL_REQUIRE(search->R >= 1 && search->R <= 1024, "%s: R=%d out of range 1..1024", fn, search->R);             \
        CRL_REQUIRE(search->cexp <= 65535u, "%s: cexp=%u out of range 0..65535", fn, search->cexp);                   \
    }

// LDS of a workgroup of the search kernels, at most 64 KB: the trees of its waves (one to four, as many as fit) behind the
// two tables.  A tree that leaves no room for a table does without it: the win test is then computed, the cell found by
// arithmetic.  win_tab: the table on this device or NULL (ttt_win_table_here); NULL comes back where it is not used.
struct ttt_mcts_geometry {
    const uint32_t *win_tab;
    int use_rank;
    uint32_t tree_words, waves, lds_bytes;
    unsigned blocks;
};
static ttt_mcts_geometry ttt_mcts_geometry_of(const crl_ctx *ctx, const int64_t B, const int S, const uint32_t *win_tab)
{
    constexpr uint32_t kLds = 65536u, kWinTab = 8192u, kRankTab = 2048u;
    const int cells = ctx->ttt.n_cells;
    const uint32_t tree_bytes = (((uint32_t)(S + 1) * (uint32_t)(8 + 2 * cells)) + 3u) & ~3u;
    if (cells > 16 || ctx->ttt_dd.n_dirs > 4 || tree_bytes + kWinTab + kRankTab > kLds) win_tab = nullptr;
    const int use_rank = tree_bytes + (win_tab ? kWinTab : 0u) + kRankTab <= kLds;
    const uint32_t tables = (win_tab ? kWinTab : 0u) + (use_rank ? kRankTab : 0u);
    uint32_t waves = (kLds - tables) / tree_bytes;
    waves = waves > 4u ? 4u : waves;
    waves = (int64_t)waves > B ? (uint32_t)B : waves;
    const uint64_t want = ((uint64_t)B + waves - 1u) / waves;
    const unsigned blocks = (unsigned)(want < (1u << 20) ? want : (1u << 20));      // (a grid-stride loop past that)
    return {win_tab, use_rank, tree_bytes / 4u, waves, tables + waves * tree_bytes, blocks};
}

static int ttt_mcts_launch(const char *fn, const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, const uint32_t *occ,
                           const int8_t *winner, const int8_t *to_move, const uint32_t *tcount, int S, int R, uint32_t cexp,
                           uint32_t *visits, uint32_t *value, uint32_t *nodes, int32_t *best, uint32_t flags, void *stream)
{
    TTT_CTX_CHECK(fn);
    CRL_REQUIRE(occ && winner && to_move, "%s: NULL state pointer", fn);
    CRL_REQUIRE(visits && value && nodes && best, "%s: NULL output pointer", fn);
    const ttt_search params = {S, R, cexp}, *search = &params;
    TTT_SEARCH_CHECK(fn);
    CRL_REQUIRE(flags == 0, "%s: unknown flags 0x%x", fn, flags);
    CRL_REQUIRE(ctx->ttt.n_cells >= ctx->ttt.P, "%s: a board of %d cells for %d players (as crl_ttt_playout)", fn, ctx->ttt.n_cells,
                ctx->ttt.P);
    const ttt_dirs dd = dirs_of(ctx);
    const ttt_mcts_geometry geo = ttt_mcts_geometry_of(ctx, B, S, ttt_win_table_here(ctx));
    const uint32_t *win_tab = geo.win_tab;
    TTT_DISPATCH_ND_WT(ctx, win_tab, hipLaunchKernelGGL((ttt_mcts_kernel<PP, NDD, WTT>), dim3(geo.blocks), dim3(64u * geo.waves),
                                                        geo.lds_bytes, (hipStream_t)stream, dd, B, (uint32_t)seed,
                                                        (uint32_t)(seed >> 32), first_env_id, occ, winner, to_move, tcount, S, R,
                                                        cexp, geo.tree_words, geo.use_rank, visits, value, nodes, best, win_tab));
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

// the search agent's kernel in one of its three frames (the entries' checks are done): ttt_mcts_launch's geometry
template <int FRAME>
static int ttt_agent_launch(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, double noise, const ttt_search &search,
                            uint32_t *occ, int8_t *winner, int8_t *to_move, const ttt_agent_io &io, void *stream)
{
    const ttt_dirs dd = dirs_of(ctx);
    const ttt_mcts_geometry geo = ttt_mcts_geometry_of(ctx, B, search.S, ttt_win_table_here(ctx));
    const uint32_t *win_tab = geo.win_tab;
    TTT_DISPATCH_ND_WT(ctx, win_tab, hipLaunchKernelGGL((ttt_mcts_agent_kernel<PP, NDD, WTT, FRAME>), dim3(geo.blocks),
                                                        dim3(64u * geo.waves), geo.lds_bytes, (hipStream_t)stream, dd, B,
                                                        (uint32_t)seed, (uint32_t)(seed >> 32), first_env_id,
                                                        crl_noise_threshold(noise), search.S, search.R, search.cexp, geo.tree_words,
                                                        geo.use_rank, occ, winner, to_move, io, win_tab));
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

// ---- one launcher per family of entries (random agent / tactical agent / search agent): `fn` names the entry in the
// messages, `noise` is NULL for the random agent's, `search` is NULL but for the search agent's
static int ttt_sample_launch(const char *fn, const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, const uint32_t *occ,
                             const int8_t *to_move, uint32_t *tcount, int advance, const double *noise, const ttt_search *search,
                             int8_t *action, void *stream)
{
    TTT_CTX_CHECK(fn);
    CRL_REQUIRE(occ && (to_move || !noise) && tcount && action, "%s: NULL pointer", fn);
    TTT_SEARCH_CHECK(fn);
    TTT_NOISE_CHECK(fn);
    const ttt_dirs dd = dirs_of(ctx);
    if (search) {
        ttt_agent_io io = {};
        io.tcount = tcount; io.action = action; io.advance = advance;
        return ttt_agent_launch<TTT_FRAME_SAMPLE>(ctx, B, seed, first_env_id, *noise, *search, const_cast<uint32_t *>(occ), nullptr,
                                                  const_cast<int8_t *>(to_move), io, stream);
    }
    if (noise) {
        TTT_DISPATCH_ND(ctx, TTT_LAUNCH((ttt_sample_tactical_kernel<PP, NDD>), blocks_for(B, 256), dd, B, (uint32_t)seed,
                                        (uint32_t)(seed >> 32), first_env_id, crl_noise_threshold(*noise), occ, to_move, tcount,
                                        advance, action));
    } else {
        TTT_LAUNCH(ttt_sample_kernel, blocks_for(B, 256), ctx->ttt.P, dd.full, B,
                   (uint32_t)seed, (uint32_t)(seed >> 32), first_env_id, occ, tcount, advance, action);
    }
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

static int ttt_step_single_launch(const char *fn, const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, uint32_t *occ,
                                  int8_t *winner, int8_t *to_move, const int8_t *seat, const int64_t *learner_action,
                                  uint32_t *tcount, int8_t *reward, uint8_t *done, int8_t *winners, int8_t *obs_board,
                                  uint32_t *valid, int rel_mod, const double *noise, const ttt_search *search, uint32_t flags,
                                  void *stream)
{
    TTT_CTX_CHECK(fn);
    CRL_REQUIRE(occ && winner && to_move, "%s: NULL state pointer", fn);
    CRL_REQUIRE(seat && tcount, "%s: NULL seat / tcount pointer", fn);
    CRL_REQUIRE(reward && done && winners && obs_board && valid, "%s: NULL output pointer", fn);
    CRL_REQUIRE(rel_mod >= 1, "%s: rel_mod must be >= 1", fn);
    TTT_SEARCH_CHECK(fn);
    TTT_NOISE_CHECK(fn);
    CRL_REQUIRE(flags == 0, "%s: unknown flags 0x%x", fn, flags);
    CRL_REQUIRE(ctx->ttt.n_cells >= ctx->ttt.P, "%s: a board of %d cells for %d players (%s)", fn, ctx->ttt.n_cells, ctx->ttt.P,
                noise ? "as crl_ttt_step_single" : "a fresh game could end before the learner's turn");
    CRL_REQUIRE((((uintptr_t)obs_board) & 3) == 0, "%s: obs_board must be 4-byte aligned", fn);
    const ttt_dirs dd = dirs_of(ctx);
    const uint32_t *win_tab = ttt_win_table_here(ctx);
    if (search) {
        ttt_agent_io io = {};
        io.tcount = tcount; io.seat = seat; io.learner_action = learner_action; io.reward = reward; io.done = done;
        io.winners = winners; io.obs = obs_board; io.valid = valid; io.rel_mod = rel_mod;
        return ttt_agent_launch<TTT_FRAME_SINGLE>(ctx, B, seed, first_env_id, *noise, *search, occ, winner, to_move, io, stream);
    }
    if (noise) {
        TTT_DISPATCH_ND_WT(ctx, win_tab, TTT_LAUNCH((ttt_step_single_tactical_kernel<PP, NDD, WTT>), blocks_for(B, 256), dd,
                                                    ttt_inv_cells(dd.n_cells), B, (uint32_t)seed, (uint32_t)(seed >> 32), first_env_id,
                                                    crl_noise_threshold(*noise), occ, winner, to_move, seat, learner_action, tcount,
                                                    reward, done, winners, obs_board, valid, rel_mod, win_tab));
    } else {
        TTT_DISPATCH_ND_WT(ctx, win_tab, TTT_LAUNCH((ttt_step_single_kernel<PP, NDD, WTT>), blocks_for(B, 256), dd,
                                                    ttt_inv_cells(dd.n_cells), B, (uint32_t)seed, (uint32_t)(seed >> 32), first_env_id,
                                                    occ, winner, to_move, seat, learner_action, tcount, reward, done, winners,
                                                    obs_board, valid, rel_mod, win_tab));
    }
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

static int ttt_playout_launch(const char *fn, const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id,
                              const uint32_t *occ, const int8_t *winner, const int8_t *to_move, const uint32_t *tcount,
                              const int32_t *cand, int A, int R, uint32_t *wins, uint32_t *played, uint32_t *len_sum,
                              const double *noise, uint32_t flags, void *stream)
{
    TTT_CTX_CHECK(fn);
    CRL_REQUIRE(occ && winner && to_move, "%s: NULL state pointer", fn);
    CRL_REQUIRE(wins && played && len_sum, "%s: NULL output pointer", fn);
    CRL_PLAYOUT_SHAPE_CHECK(fn);
    TTT_NOISE_CHECK(fn);
    CRL_REQUIRE(flags == 0, "%s: unknown flags 0x%x", fn, flags);
    CRL_REQUIRE(ctx->ttt.n_cells >= ctx->ttt.P, "%s: a board of %d cells for %d players (as crl_ttt_step_single)", fn,
                ctx->ttt.n_cells, ctx->ttt.P);
    const ttt_dirs dd = dirs_of(ctx);
    const uint32_t *win_tab = ttt_win_table_here(ctx);
    const auto [rows, n_lanes] = crl_playout_shape_of(B, A, R);
    // rows that span waves are summed by atomics: every output starts from zero
    CRL_HIP(hipMemsetAsync(wins, 0, rows * ctx->ttt.P * sizeof(uint32_t), (hipStream_t)stream));
    CRL_HIP(hipMemsetAsync(played, 0, rows * sizeof(uint32_t), (hipStream_t)stream));
    CRL_HIP(hipMemsetAsync(len_sum, 0, rows * sizeof(uint32_t), (hipStream_t)stream));
    const unsigned blocks = crl_playout_blocks(n_lanes, 256u);
    if (noise) {
        TTT_DISPATCH_ND_WT(ctx, win_tab, TTT_LAUNCH((ttt_playout_tactical_kernel<PP, NDD, WTT>), blocks, dd, B, (uint32_t)seed,
                                                    (uint32_t)(seed >> 32), first_env_id, crl_noise_threshold(*noise), occ, winner,
                                                    to_move, tcount, cand, A, R, n_lanes, wins, played, len_sum, win_tab));
    } else {
        TTT_DISPATCH_ND_WT(ctx, win_tab, TTT_LAUNCH((ttt_playout_kernel<PP, NDD, WTT>), blocks, dd, B, (uint32_t)seed,
                                                    (uint32_t)(seed >> 32), first_env_id, occ, winner, to_move, tcount, cand, A, R,
                                                    n_lanes, wins, played, len_sum, win_tab));
    }
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

// The arguments of crl_ttt_rollout that stay the same from launch to launch (include/colosseum_hip.h, "launch plans"), checked.
// The win table is looked up per launch: it depends on the device that is current then.
struct ttt_plan : crl_plan {
    const crl_ctx *ctx;
    int64_t B;
    uint64_t first_env_id;
    uint32_t *occ;
    int8_t *winner, *to_move;
    crl_ttt_stats st;
    ttt_dirs dd;

    int run(const char *fn, uint64_t seed, int T, const double *noise, const ttt_search *search, void *stream) const;
    int launch(uint64_t seed, int T, void *stream) const override { return run("crl_rollout_launch", seed, T, nullptr, nullptr, stream); }
};

static int ttt_plan_bind(ttt_plan &p, const char *fn, const crl_ctx *ctx, int64_t B, uint64_t first_env_id, uint32_t *occ,
                         int8_t *winner, int8_t *to_move, const crl_ttt_stats &st)
{
    TTT_CTX_CHECK(fn);
    CRL_REQUIRE(occ && winner && to_move, "%s: NULL state pointer", fn);
    CRL_REQUIRE(st.tcount && st.tstep && st.n_episodes && st.win_count && st.draw_count && st.len_sum, "%s: NULL stats pointer", fn);
    p.ctx = ctx; p.B = B; p.first_env_id = first_env_id;
    p.occ = occ; p.winner = winner; p.to_move = to_move;
    p.st = st;
    p.dd = dirs_of(ctx);
    return CRL_OK;
}

int ttt_plan::run(const char *fn, const uint64_t seed, const int T, const double *noise, const ttt_search *search, void *stream) const
{
    CRL_REQUIRE(T >= 0 && T <= (1 << 24), "%s: T=%d out of range", fn, T);
    TTT_SEARCH_CHECK(fn);
    TTT_NOISE_CHECK(fn);
    if (T == 0) return CRL_OK;
    const uint32_t *win_tab = ttt_win_table_here(ctx);
    if (search) {
        ttt_agent_io io = {};
        io.T = T; io.st = st;
        return ttt_agent_launch<TTT_FRAME_ROLLOUT>(ctx, B, seed, first_env_id, *noise, *search, occ, winner, to_move, io, stream);
    }
    if (noise) {
        TTT_DISPATCH_ND_WT(ctx, win_tab, TTT_LAUNCH((ttt_rollout_tactical_kernel<PP, NDD, WTT>), blocks_for(B, 256), dd, B,
                                                    (uint32_t)seed, (uint32_t)(seed >> 32), first_env_id, crl_noise_threshold(*noise),
                                                    T, occ, winner, to_move, st, win_tab));
    } else {
        TTT_DISPATCH_ND_WT(ctx, win_tab, TTT_LAUNCH((ttt_rollout_kernel<PP, NDD, WTT>), blocks_for(B, 256), dd, B, (uint32_t)seed,
                                                    (uint32_t)(seed >> 32), first_env_id, T, occ, winner, to_move, st, win_tab));
    }
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

static int ttt_rollout_launch(const char *fn, const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, int T,
                              const double *noise, const ttt_search *search, uint32_t *occ, int8_t *winner, int8_t *to_move,
                              crl_ttt_stats st, void *stream)
{
    ttt_plan plan;
    if (const int rc = ttt_plan_bind(plan, fn, ctx, B, first_env_id, occ, winner, to_move, st)) return rc;
    return plan.run(fn, seed, T, noise, search, stream);
}

extern "C" {

int crl_ttt_create(int D0, int D1, int D2, int K, int P, crl_ctx **out)
{
    CRL_REQUIRE(out != nullptr, "crl_ttt_create: out is NULL");
    CRL_REQUIRE(D0 >= 1 && D1 >= 1 && D2 >= 1 && (int64_t)D0 * D1 * D2 <= 32, "crl_ttt_create: board %dx%dx%d must have 1..32 cells", D0, D1, D2);
    CRL_REQUIRE(K >= 2 && K <= 32, "crl_ttt_create: K=%d out of range", K);
    CRL_REQUIRE(P >= 1 && P <= CRL_TTT_MAX_P, "crl_ttt_create: P=%d out of range 1..%d", P, CRL_TTT_MAX_P);
    crl_ctx *c = new crl_ctx();
    memset(c, 0, sizeof(*c));
    c->game = CRL_GAME_TTT;
    c->ttt.D0 = D0; c->ttt.D1 = D1; c->ttt.D2 = D2; c->ttt.K = K; c->ttt.P = P;
    c->ttt.n_cells = D0 * D1 * D2;
    c->ttt.full = c->ttt.n_cells == 32 ? 0xffffffffu : ((1u << c->ttt.n_cells) - 1u);
    ttt_dirs dd;
    int n_lines = 0;
    if (build_dirs(c->ttt, dd, c->ttt_lines_host, n_lines) != 0) {
        delete c;
        crl_set_error("crl_ttt_create: too many win lines for %dx%dx%d K=%d", D0, D1, D2, K);
        return CRL_EUNSUPPORTED;
    }
    c->ttt.n_lines = n_lines;
    c->ttt_dd = dd;
    // Boards of at most 16 cells (the reference's 3x3 and 3x5 among them): "does this mask hold a K-line" for all 65,536
    // masks as a bit table on the device, which crl_ttt_rollout stages into LDS -- one LDS read and four vector
    // instructions per ply instead of the four-direction shift-and test.  Optional: without it (no device at create
    // time, or a rollout on another device) the rollout computes the test as everywhere else.
    if (c->ttt.n_cells <= 16 && getenv("CRL_TTT_NO_WIN_TABLE") == nullptr) {     // (the switch: tests of the table-less path)
        std::vector<uint32_t> tab(2048, 0u);
        for (uint32_t m = 0; m < 65536u; ++m)
            for (int i = 0; i < n_lines; ++i)
                if ((m & c->ttt_lines_host[i]) == c->ttt_lines_host[i]) { tab[m >> 5] |= 1u << (m & 31u); break; }
        int dev = -1;
        void *d = nullptr;
        if (hipGetDevice(&dev) == hipSuccess && hipMalloc(&d, tab.size() * sizeof(uint32_t)) == hipSuccess) {
            if (hipMemcpy(d, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess) {
                c->ttt_win_dev = (uint32_t *)d;
                c->ttt_win_device = dev;
            } else {
                (void)hipFree(d);
            }
        }
        (void)hipGetLastError();                           // (a failure here is not an error of the call)
    }
    *out = c;
    return CRL_OK;
}

int crl_ttt_lines(const crl_ctx *ctx, uint32_t *lines, int cap)
{
    CRL_REQUIRE(ctx != nullptr && ctx->game == CRL_GAME_TTT, "crl_ttt_lines: ctx is not a tictactoe context");
    if (lines)
        for (int i = 0; i < ctx->ttt.n_lines && i < cap; ++i) lines[i] = ctx->ttt_lines_host[i];
    return ctx->ttt.n_lines;
}

int crl_ttt_reset(const crl_ctx *ctx, int64_t B, const uint8_t *mask, uint32_t *occ, int8_t *winner, int8_t *to_move, void *stream)
{
    TTT_CTX_CHECK("crl_ttt_reset");
    CRL_REQUIRE(occ && winner && to_move, "crl_ttt_reset: NULL state pointer");
    TTT_LAUNCH(ttt_reset_kernel, blocks_for(B, 256), ctx->ttt.P, B, mask, occ, winner, to_move);
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

int crl_ttt_step(const crl_ctx *ctx, int64_t B, uint32_t *occ, int8_t *winner, int8_t *to_move,
                 const int8_t *action, int8_t *reward, uint8_t *terminal, int8_t *winners, uint32_t flags, void *stream)
{
    TTT_CTX_CHECK("crl_ttt_step");
    CRL_REQUIRE(occ && winner && to_move, "crl_ttt_step: NULL state pointer");
    CRL_REQUIRE(action && reward && terminal && winners, "crl_ttt_step: NULL action/output pointer");
    CRL_REQUIRE((flags & ~CRL_STEP_AUTO_RESET) == 0, "crl_ttt_step: unknown flags 0x%x", flags);
    const ttt_dirs dd = dirs_of(ctx);
    TTT_DISPATCH_ND(ctx, TTT_LAUNCH((ttt_step_kernel<PP, NDD>), blocks_for(B, 256), dd, B, occ, winner, to_move, action, reward,
                                    terminal, winners, flags));
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

int crl_ttt_valid(const crl_ctx *ctx, int64_t B, const uint32_t *occ, uint32_t *valid, void *stream)
{
    TTT_CTX_CHECK("crl_ttt_valid");
    CRL_REQUIRE(occ && valid, "crl_ttt_valid: NULL pointer");
    TTT_LAUNCH(ttt_valid_kernel, blocks_for(B, 256), ctx->ttt.P, ctx->ttt.full, B, occ, valid);
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

int crl_ttt_board(const crl_ctx *ctx, int64_t B, const uint32_t *occ, const int8_t *player, int rel_mod, int8_t *board, void *stream)
{
    TTT_CTX_CHECK("crl_ttt_board");
    CRL_REQUIRE(occ && board, "crl_ttt_board: NULL pointer");
    CRL_REQUIRE(player == nullptr || rel_mod >= 1, "crl_ttt_board: rel_mod must be >= 1 when player is given");
    CRL_REQUIRE((((uintptr_t)board) & 3) == 0, "crl_ttt_board: board must be 4-byte aligned");
    const int cells = ctx->ttt.n_cells;
    TTT_DISPATCH_P(ctx->ttt.P, TTT_LAUNCH((ttt_board_kernel<PP>), blocks_for(B, 256), cells, ttt_inv_cells(cells), B, occ, player,
                                          rel_mod < 1 ? 1 : rel_mod, board));
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

int crl_ttt_sample(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, const uint32_t *occ, uint32_t *tcount,
                   int advance, int8_t *action, void *stream)
{
    return ttt_sample_launch("crl_ttt_sample", ctx, B, seed, first_env_id, occ, nullptr, tcount, advance, nullptr, nullptr, action, stream);
}

int crl_ttt_step_observe(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id,
                         uint32_t *occ, int8_t *winner, int8_t *to_move, const int8_t *action, uint32_t *tcount,
                         int8_t *reward, uint8_t *terminal, int8_t *winners, int8_t *obs_board, uint32_t *valid,
                         int rel_mod, uint32_t flags, void *stream)
{
    TTT_CTX_CHECK("crl_ttt_step_observe");
    CRL_REQUIRE(occ && winner && to_move, "crl_ttt_step_observe: NULL state pointer");
    CRL_REQUIRE(action || tcount, "crl_ttt_step_observe: action and tcount are both NULL (nothing to play)");
    CRL_REQUIRE(reward && terminal && winners && obs_board && valid, "crl_ttt_step_observe: NULL output pointer");
    CRL_REQUIRE(rel_mod >= 1, "crl_ttt_step_observe: rel_mod must be >= 1");
    CRL_REQUIRE((flags & ~CRL_STEP_AUTO_RESET) == 0, "crl_ttt_step_observe: unknown flags 0x%x", flags);
    CRL_REQUIRE((((uintptr_t)obs_board) & 3) == 0, "crl_ttt_step_observe: obs_board must be 4-byte aligned");
    const ttt_dirs dd = dirs_of(ctx);
    TTT_DISPATCH_ND(ctx, TTT_LAUNCH((ttt_step_observe_kernel<PP, NDD>), blocks_for(B, 256), dd, ttt_inv_cells(dd.n_cells), B,
                                    (uint32_t)seed, (uint32_t)(seed >> 32), first_env_id, occ, winner, to_move, action, tcount,
                                    reward, terminal, winners, obs_board, valid, rel_mod, flags));
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

int crl_ttt_step_single(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, uint32_t *occ, int8_t *winner,
                        int8_t *to_move, const int8_t *seat, const int64_t *learner_action, uint32_t *tcount, int8_t *reward,
                        uint8_t *done, int8_t *winners, int8_t *obs_board, uint32_t *valid, int rel_mod, uint32_t flags, void *stream)
{
    return ttt_step_single_launch("crl_ttt_step_single", ctx, B, seed, first_env_id, occ, winner, to_move, seat, learner_action, tcount,
                                  reward, done, winners, obs_board, valid, rel_mod, nullptr, nullptr, flags, stream);
}

int crl_ttt_playout(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, const uint32_t *occ, const int8_t *winner,
                    const int8_t *to_move, const uint32_t *tcount, const int32_t *cand, int A, int R, uint32_t *wins,
                    uint32_t *played, uint32_t *len_sum, uint32_t flags, void *stream)
{
    return ttt_playout_launch("crl_ttt_playout", ctx, B, seed, first_env_id, occ, winner, to_move, tcount, cand, A, R, wins, played,
                              len_sum, nullptr, flags, stream);
}

int crl_ttt_mcts_max_simulations(const crl_ctx *ctx)
{
    CRL_REQUIRE(ctx != nullptr && ctx->game == CRL_GAME_TTT, "crl_ttt_mcts_max_simulations: ctx is not a tictactoe context");
    return ttt_mcts_max_simulations(ctx->ttt.n_cells);
}

int crl_ttt_mcts(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, const uint32_t *occ, const int8_t *winner,
                 const int8_t *to_move, const uint32_t *tcount, int S, int R, uint32_t cexp, uint32_t *visits, uint32_t *value,
                 uint32_t *nodes, int32_t *best, uint32_t flags, void *stream)
{
    return ttt_mcts_launch("crl_ttt_mcts", ctx, B, seed, first_env_id, occ, winner, to_move, tcount, S, R, cexp, visits, value, nodes,
                           best, flags, stream);
}

static int ttt_step_board_launch(const char *fn, const crl_ctx *ctx, int64_t B, int8_t *board, int8_t *winner, int8_t *to_move,
                                 const int8_t *action, int8_t *reward, uint8_t *terminal, int8_t *winners, uint32_t *valid,
                                 int8_t *obs_board, int rel_mod, uint32_t flags, void *stream, const bool by_value, uint32_t *flag,
                                 const uint32_t seq)
{
    TTT_CTX_CHECK(fn);
    CRL_REQUIRE(board && winner && to_move, "%s: NULL state pointer", fn);
    CRL_REQUIRE(action && reward && terminal && winners, "%s: NULL action/output pointer", fn);
    CRL_REQUIRE(obs_board == nullptr || rel_mod >= 1, "%s: rel_mod must be >= 1 when obs_board is given", fn);
    CRL_REQUIRE((flags & ~CRL_STEP_AUTO_RESET) == 0, "%s: unknown flags 0x%x", fn, flags);
    const ttt_dirs dd = dirs_of(ctx);
    const int rm = rel_mod < 1 ? 1 : rel_mod;
    TttVec vec = {};
    if (by_value) {                                             // host-visible state (crl_host_alloc): read here, passed as arguments
        for (int c = 0; c < dd.n_cells; ++c) {
            const int v = board[c];
            if (v >= 0 && v < ctx->ttt.P) vec.occ[v] |= 1u << c;
        }
        vec.winner = winner[0]; vec.to_move = to_move[0]; vec.action = action[0];
    }
    TTT_DISPATCH_ND(ctx, TTT_LAUNCH((ttt_step_board_kernel<PP, NDD>), blocks_for(B, 256), dd, B, board, winner, to_move, action,
                                    reward, terminal, winners, valid, obs_board, rm, flags, vec, by_value, flag, seq));
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

int crl_ttt_step_board(const crl_ctx *ctx, int64_t B, int8_t *board, int8_t *winner, int8_t *to_move, const int8_t *action,
                       int8_t *reward, uint8_t *terminal, int8_t *winners, uint32_t *valid, int8_t *obs_board, int rel_mod,
                       uint32_t flags, void *stream)
{
    return ttt_step_board_launch("crl_ttt_step_board", ctx, B, board, winner, to_move, action, reward, terminal, winners, valid,
                                 obs_board, rel_mod, flags, stream, false, nullptr, 0u);
}

int crl_ttt_step_board_host(const crl_ctx *ctx, int8_t *board, int8_t *winner, int8_t *to_move, const int8_t *action,
                            int8_t *reward, uint8_t *terminal, int8_t *winners, uint32_t *valid, int8_t *obs_board, int rel_mod,
                            uint32_t flags, void *stream, uint32_t *flag, uint32_t seq, double timeout_s)
{
    CRL_REQUIRE(flag != nullptr, "crl_ttt_step_board_host: flag is NULL");
    const int rc = ttt_step_board_launch("crl_ttt_step_board_host", ctx, 1, board, winner, to_move, action, reward, terminal, winners,
                                         valid, obs_board, rel_mod, flags, stream, true, flag, seq);
    if (rc != CRL_OK) return rc;
    return crl_spin_mapped(stream, flag, seq, timeout_s, "crl_ttt_step_board_host");
}

int crl_ttt_observe_board(const crl_ctx *ctx, int64_t B, const int8_t *board, const int8_t *player, int rel_mod,
                          int8_t *obs_board, uint32_t *valid, void *stream)
{
    TTT_CTX_CHECK("crl_ttt_observe_board");
    CRL_REQUIRE(board != nullptr, "crl_ttt_observe_board: board is NULL");
    CRL_REQUIRE(obs_board || valid, "crl_ttt_observe_board: nothing to compute (obs_board and valid are NULL)");
    CRL_REQUIRE(player == nullptr || rel_mod >= 1, "crl_ttt_observe_board: rel_mod must be >= 1 when player is given");
    TTT_DISPATCH_P(ctx->ttt.P, TTT_LAUNCH((ttt_observe_board_kernel<PP>), blocks_for(B, 256), ctx->ttt.n_cells, ctx->ttt.full, B,
                                          board, player, rel_mod < 1 ? 1 : rel_mod, obs_board, valid));
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

int crl_ttt_rollout(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, int T, uint32_t *occ, int8_t *winner,
                    int8_t *to_move, crl_ttt_stats st, void *stream)
{
    return ttt_rollout_launch("crl_ttt_rollout", ctx, B, seed, first_env_id, T, nullptr, nullptr, occ, winner, to_move, st, stream);
}

int crl_ttt_rollout_bind(const crl_ctx *ctx, int64_t B, uint64_t first_env_id, uint32_t *occ, int8_t *winner, int8_t *to_move,
                         crl_ttt_stats st, crl_plan **out)
{
    CRL_REQUIRE(out != nullptr, "crl_ttt_rollout_bind: plan is NULL");
    *out = nullptr;
    ttt_plan *plan = new ttt_plan();
    if (const int rc = ttt_plan_bind(*plan, "crl_ttt_rollout_bind", ctx, B, first_env_id, occ, winner, to_move, st)) {
        delete plan;
        return rc;
    }
    *out = plan;
    return CRL_OK;
}

// ---- the tactical agent's entries (the contract is in include/colosseum_hip.h)
int crl_ttt_winning_cells(const crl_ctx *ctx, int64_t B, const uint32_t *occ, uint32_t *cells, void *stream)
{
    TTT_CTX_CHECK("crl_ttt_winning_cells");
    CRL_REQUIRE(occ && cells, "crl_ttt_winning_cells: NULL pointer");
    const ttt_dirs dd = dirs_of(ctx);
    TTT_DISPATCH_ND(ctx, TTT_LAUNCH((ttt_winning_cells_kernel<PP, NDD>), blocks_for(B, 256), dd, B, occ, cells));
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

int crl_ttt_sample_tactical(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, const uint32_t *occ,
                            const int8_t *to_move, uint32_t *tcount, int advance, double noise, int8_t *action, void *stream)
{
    return ttt_sample_launch("crl_ttt_sample_tactical", ctx, B, seed, first_env_id, occ, to_move, tcount, advance, &noise, nullptr,
                             action, stream);
}

int crl_ttt_rollout_tactical(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, int T, double noise, uint32_t *occ,
                             int8_t *winner, int8_t *to_move, crl_ttt_stats st, void *stream)
{
    return ttt_rollout_launch("crl_ttt_rollout_tactical", ctx, B, seed, first_env_id, T, &noise, nullptr, occ, winner, to_move, st, stream);
}

int crl_ttt_step_single_tactical(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, uint32_t *occ, int8_t *winner,
                                 int8_t *to_move, const int8_t *seat, const int64_t *learner_action, uint32_t *tcount, int8_t *reward,
                                 uint8_t *done, int8_t *winners, int8_t *obs_board, uint32_t *valid, int rel_mod, double noise,
                                 uint32_t flags, void *stream)
{
    return ttt_step_single_launch("crl_ttt_step_single_tactical", ctx, B, seed, first_env_id, occ, winner, to_move, seat,
                                  learner_action, tcount, reward, done, winners, obs_board, valid, rel_mod, &noise, nullptr, flags,
                                  stream);
}

int crl_ttt_playout_tactical(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, const uint32_t *occ,
                             const int8_t *winner, const int8_t *to_move, const uint32_t *tcount, const int32_t *cand, int A, int R,
                             uint32_t *wins, uint32_t *played, uint32_t *len_sum, double noise, uint32_t flags, void *stream)
{
    return ttt_playout_launch("crl_ttt_playout_tactical", ctx, B, seed, first_env_id, occ, winner, to_move, tcount, cand, A, R, wins,
                              played, len_sum, &noise, flags, stream);
}

// ---- the search agent's entries (the contract is in include/colosseum_hip.h)
int crl_ttt_sample_mcts(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, const uint32_t *occ,
                        const int8_t *to_move, uint32_t *tcount, int advance, int S, int R, uint32_t cexp, double noise,
                        int8_t *action, void *stream)
{
    const ttt_search search = {S, R, cexp};
    return ttt_sample_launch("crl_ttt_sample_mcts", ctx, B, seed, first_env_id, occ, to_move, tcount, advance, &noise, &search, action,
                             stream);
}

int crl_ttt_rollout_mcts(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, int T, int S, int R, uint32_t cexp,
                         double noise, uint32_t *occ, int8_t *winner, int8_t *to_move, crl_ttt_stats st, void *stream)
{
    const ttt_search search = {S, R, cexp};
    return ttt_rollout_launch("crl_ttt_rollout_mcts", ctx, B, seed, first_env_id, T, &noise, &search, occ, winner, to_move, st, stream);
}

int crl_ttt_step_single_mcts(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, uint32_t *occ, int8_t *winner,
                             int8_t *to_move, const int8_t *seat, const int64_t *learner_action, uint32_t *tcount, int8_t *reward,
                             uint8_t *done, int8_t *winners, int8_t *obs_board, uint32_t *valid, int rel_mod, int S, int R,
                             uint32_t cexp, double noise, uint32_t flags, void *stream)
{
    const ttt_search search = {S, R, cexp};
    return ttt_step_single_launch("crl_ttt_step_single_mcts", ctx, B, seed, first_env_id, occ, winner, to_move, seat, learner_action,
                                  tcount, reward, done, winners, obs_board, valid, rel_mod, &noise, &search, flags, stream);
}

} // extern "C"

#endif // TTT_DEVICE_ONLY (the entries)
