// tron_mcts.hip -- batched tree search (UCT) for one seat of Tron, one tree per wave (crl_tron_mcts,
// crl_tron_mcts_max_simulations).  Contract: include/colosseum_hip.h, beside crl_tron_playout; DESIGN.md section 4.5e.
//
// The tree branches on the seat's three actions only; every other player is part of the transition (a scripted model drawn
// from counter-based streams), so a node's position is a function of the root and the edge sequence and a node needs three
// child slots, no position.  The mapping follows ttt_mcts_kernel (ttt.hip): a wave owns a tree in LDS and walks its games in
// a grid-stride loop; the descent is wave-uniform (the player vectors are alike in every lane, the working bitboard is one
// copy in LDS that every lane reads at the same address and rewrites with the same word); while the wave selects, lanes
// 0..2 are the three children; while it evaluates, lane r is playout r on a private bitboard; while it backs up, lane i is
// entry i of the path.  Lanes hand values to each other through LDS only across tm_wave_sync.
//
// The playout step and the avoid decision of tron.hip sit in that file's anonymous namespace; they are restated here (as
// tron_territory.hip restates the bitboard build), from the contract of crl_tron_playout / crl_tron_sample_avoid.
//
// LDS of a workgroup of W waves (one to four), in dwords, nwords = ceil(N*N / 32):
//   [the playout bitboards: word w of slot k at w * (64 W) + k, slot = 64 wave + lane   (tron_playout_kernel's layout)]
//   [per wave: n[S + 1] | w[S + 1] | child uint16 [S + 1][3], 0 = none | path uint16 [S + 1] | root[nwords] | work[nwords]]
// 16 (S + 1) + 264 nwords bytes per wave, which is what bounds S (tron_mcts_max_simulations below).
//
// crl_tron_mcts_territory is the same search with one Voronoi flood of the leaf's position in the
// place of the playouts: tron_mcts_territory_kernel below, without the playout bitboards (16 (S + 1) + 8 nwords bytes per wave).
// crl_tron_sample_mcts_territory seats that search at the players of a mask:
// tron_sample_mcts_territory_kernel, one workgroup per game, one wave and one such slice of LDS per masked player.
#include "crl_common.hpp"

namespace {

__device__ __forceinline__ void tm_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// floor(num / den) for num < 2^52 and 1 <= den < 2^32: the double quotient is within one of it, the remainder decides
__device__ __forceinline__ uint64_t tm_div(const uint64_t num, const uint32_t den)
{
    uint64_t q = (uint64_t)((double)num / (double)den);
    const int64_t r = (int64_t)(num - q * (uint64_t)den);
    q = r < 0 ? q - 1u : (r >= (int64_t)den ? q + 1u : q);
    return q;
}

// the exact floor square root of x < 2^52
__device__ __forceinline__ uint64_t tm_isqrt(const uint64_t x)
{
    uint64_t s = (uint64_t)sqrt((double)x);
    s = s * s > x ? s - 1u : ((s + 1u) * (s + 1u) <= x ? s + 1u : s);
    return s;
}

// the contract's piecewise-linear log2 with 8 fraction bits, n >= 1
__device__ __forceinline__ uint32_t tm_lg(const uint32_t n)
{
    const uint32_t m = 31u - (uint32_t)__clz((int)n);
    return 256u * m + (((n << (31u - m)) >> 23) & 255u);
}

// bit 7 of each byte: the byte is in 1..127 (> 0 as int8); then bits 7, 15, 23, 31 -> bits 0..3
__device__ __forceinline__ uint32_t tm_occ_nibble(const uint32_t x)
{
    const uint32_t m = ((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) & ~x & 0x80808080u;
    return (((m >> 7) * 0x00204081u) >> 21) & 0xfu;
}

// occupancy of the n <= 32 cells from p on: bit i set iff p[i] > 0.  Aligned dword loads, each holding at least one byte of
// the run (so none leaves the pages the run lies in).
__device__ __forceinline__ uint32_t tm_occ_run(const int8_t *p, const int n)
{
    const uintptr_t addr = reinterpret_cast<uintptr_t>(p);
    const uint32_t off = (uint32_t)(addr & 3u);
    const uint32_t *src = reinterpret_cast<const uint32_t *>(addr - off);
    const int nd = (n + (int)off + 3) >> 2;
    uint64_t acc = tm_occ_nibble(src[0]) >> off;
    int fill = 4 - (int)off;
    for (int i = 1; i < nd; ++i) {                              // (fill <= 36: n <= 32)
        acc |= (uint64_t)tm_occ_nibble(src[i]) << fill;
        fill += 4;
    }
    return n >= 32 ? (uint32_t)acc : (uint32_t)acc & ((1u << n) - 1u);
}

// a position without its board: heads (flat and split), directions, the alive mask
template <int P>
struct TmPos {
    int h[P], x[P], y[P], d[P];
    uint32_t alive;
};

// a bitboard in LDS: word w at bits[w * stride + slot]; `lim` bounds the index (the bounds build checks it)
struct TmBoard {
    uint32_t *bits;
    int stride, slot, lim;
    __device__ __forceinline__ int at(const int cell, const int code) const
    {
        const int i = (cell >> 5) * stride + slot;
        CRL_BOUNDS_LT(i, lim, code);
        (void)code;
        return i;
    }
};

// the cell next to (hx, hy) in direction dir, clamped onto the board (TronGridEnvironment.py:467-481)
__device__ __forceinline__ int tm_avoid_cell(const int N, const int hx, const int hy, const int dir)
{
    const int dd = dir & 3;
    const int nx = min(max(hx + (dd == 1) - (dd == 3), 0), N - 1);
    const int ny = min(max(hy + (dd == 2) - (dd == 0), 0), N - 1);
    return ny * N + nx;
}

// crl_tron_sample_avoid's rule for every live player on the pre-step bitboard, under the avoid playout tag with third
// counter word c2: code 0 forward, 1 right, 3 left (the step's encoding); dead players get 0
template <int P>
__device__ __forceinline__ void tm_avoid_codes(const int N, const TmBoard &bd, const TmPos<P> &s, const uint32_t gid, const uint32_t c,
                                               const uint32_t c2, const uint32_t k0, const uint32_t k1, const uint64_t thr,
                                               int (&code)[P])
{
#pragma unroll
    for (int p = 0; p < P; ++p) {
        code[p] = 0;
        if ((s.alive >> p) & 1u) {
            const int c_f = tm_avoid_cell(N, s.x[p], s.y[p], s.d[p]);
            const int c_r = tm_avoid_cell(N, s.x[p], s.y[p], s.d[p] + 1);
            const int c_l = tm_avoid_cell(N, s.x[p], s.y[p], s.d[p] + 3);
            const int o_f = (bd.bits[bd.at(c_f, 170)] >> (c_f & 31)) & 1;
            const int o_r = (bd.bits[bd.at(c_r, 171)] >> (c_r & 31)) & 1;
            const int o_l = (bd.bits[bd.at(c_l, 172)] >> (c_l & 31)) & 1;
            const philox_out wv = philox4x32_10(gid, c, c2, CRL_TAG_TRON_AVOID_PLAYOUT | (uint32_t)p, k0, k1);
            const uint32_t a3 = __umulhi(wv.w[1], 3u);
            const bool left_first = (wv.w[2] >> 31) != 0u;
            const bool first_free = (left_first ? o_l : o_r) == 0;
            const int side = (left_first == first_free) ? 3 : 1;
            code[p] = ((uint64_t)wv.w[0] < thr) ? (int)(a3 + (a3 >> 1)) : (o_f == 0 ? 0 : side);
        }
    }
}

// the random agent's Philox blocks of the 8 steps around counter c (players 0..3 and, with P > 4, players 4..7)
struct TmDraw { uint32_t a0, a1, a2, a3, b0, b1, b2, b3; };

template <int P>
__device__ __forceinline__ void tm_random_refill(const uint32_t gid, const uint32_t c, const uint32_t c2, const uint32_t k0,
                                                 const uint32_t k1, TmDraw &dr)
{
    const philox_out wv = philox4x32_10(gid, c >> 3, c2, CRL_TAG_TRON_PLAYOUT, k0, k1);
    dr.a0 = wv.w[0]; dr.a1 = wv.w[1]; dr.a2 = wv.w[2]; dr.a3 = wv.w[3];
    if constexpr (P > 4) {
        const philox_out wu = philox4x32_10(gid, c >> 3, c2, CRL_TAG_TRON_PLAYOUT | 1u, k0, k1);
        dr.b0 = wu.w[0]; dr.b1 = wu.w[1]; dr.b2 = wu.w[2]; dr.b3 = wu.w[3];
    }
}

// crl_tron_rollout's digit rule with j = c & 7: a code for every player (the dead ones' are not used)
template <int P>
__device__ __forceinline__ void tm_random_codes(const uint32_t c, const TmDraw &dr, int (&code)[P])
{
    const uint32_t sel = (c & 7u) >> 1;
    const uint32_t word_a = sel == 0u ? dr.a0 : sel == 1u ? dr.a1 : sel == 2u ? dr.a2 : dr.a3;
    const uint32_t word_b = sel == 0u ? dr.b0 : sel == 1u ? dr.b1 : sel == 2u ? dr.b2 : dr.b3;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const uint32_t lo3 =(p & 3) == 0 ? 1u : (p & 3) == 1 ? 3u : (p & 3) == 2 ? 9u : 27u;     // 3^(p & 3), 3^(4 + (p & 3))
        const uint32_t v = (p < 4 ? word_a : word_b) * ((c & 1u) ? 81u * lo3 : lo3);
        const uint32_t a3 = __umulhi(v, 3u);
        code[p] = (int)(a3 + (a3 >> 1));
    }
}

// crl_tron_step without reset on a bitboard, in the reference's sequential order (CyTronGrid.pyx:15-62): straight-line
// selects, one LDS read and write per player (rewriting an unchanged word is harmless: the board is the caller's own)
template <int P>
__device__ __forceinline__ void tm_step(const int N, const TmBoard &bd, TmPos<P> &s, const int (&code)[P])
{
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const bool run = (s.alive >> i) & 1u;                   // (may have been killed head-on by j < i)
        const int dir = (s.d[i] + code[i]) & 3;
        s.d[i] = run ? dir : s.d[i];
        const int nx = s.x[i] + (dir == 1) - (dir == 3);
        const int ny = s.y[i] + (dir == 2) - (dir == 0);
        const bool oob = (unsigned)nx >= (unsigned)N || (unsigned)ny >= (unsigned)N;
        const int cell = oob ? s.h[i] : ny * N + nx;
        const int wi = bd.at(cell, 173);
        const uint32_t word = bd.bits[wi], bit = 1u << (cell & 31);
        const bool occupied = (word & bit) != 0u;
        const bool crash = run & !oob & occupied;               // I die; the head-on owner dies too
        const bool moved = run & !oob & !occupied;
        s.alive &= ~((uint32_t)(run & (oob | occupied)) << i);
#pragma unroll
        for (int o = 0; o < P; ++o)
            if (o != i) s.alive &= ~((uint32_t)(crash & (s.h[o] == cell)) << o);
        bd.bits[wi] = moved ? (word | bit) : word;
        s.h[i] = moved ? cell : s.h[i];
        s.x[i] = moved ? nx : s.x[i];
        s.y[i] = moved ? ny : s.y[i];
    }
}

template <int P, bool AVOID>
__global__ void __launch_bounds__(256)
tron_mcts_kernel(const int N, const int NN, const uint32_t inv_n, const int64_t B, const uint32_t seed_lo, const uint32_t seed_hi,
                 const uint64_t first_env_id, const int8_t *__restrict__ board, const int16_t *__restrict__ heads,
                 const int8_t *__restrict__ dirs, const int8_t *__restrict__ deaths, const uint32_t *__restrict__ tcount,
                 const int8_t *__restrict__ seat_in, const int S, const int R, const uint32_t cexp, const uint64_t thr,
                 const int max_steps, const int nwords, const uint32_t wave_words, uint32_t *__restrict__ visits,
                 uint32_t *__restrict__ value, uint32_t *__restrict__ nodes, int32_t *__restrict__ best)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t tm_lds[];
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), n_waves = (int)(blockDim.x >> 6);
    const int nslots = n_waves * 64;
    uint32_t *n_arr = tm_lds + (uint32_t)nwords * (uint32_t)nslots + (uint32_t)wave * wave_words, *w_arr = n_arr + (S + 1);
    uint16_t *child = reinterpret_cast<uint16_t *>(w_arr + (S + 1)), *path = child + 3 * (S + 1);
    uint32_t *root_bits = w_arr + 3 * (S + 1), *work_bits = root_bits + nwords;
    const TmBoard work = {work_bits, 1, 0, nwords};
    const TmBoard mine = {tm_lds, nslots, wave * 64 + lane, nwords * nslots};
    constexpr uint32_t kTreeStep = 0xFFFF0000u;                 // the third counter word of the tree steps' draws

    for (int64_t b = (int64_t)blockIdx.x * n_waves + wave; b < B; b += (int64_t)gridDim.x * n_waves) {
        // ---- the root position, alike in every lane
        const int sp = seat_in ? __builtin_amdgcn_readfirstlane((int)seat_in[b]) : 0;
        TmPos<P> p0;
        p0.alive = 0u;
#pragma unroll
        for (int p = 0; p < P; ++p) {
            p0.h[p] = min(max(__builtin_amdgcn_readfirstlane((int)heads[p * B + b]), 0), NN - 1);   // (a broken state: wrong results, no wild access)
            p0.y[p] = (int)__umulhi((uint32_t)p0.h[p], inv_n);
            p0.x[p] = p0.h[p] - p0.y[p] * N;
            p0.d[p] = __builtin_amdgcn_readfirstlane((int)dirs[p * B + b]) & 3;
            p0.alive |= (__builtin_amdgcn_readfirstlane((int)deaths[p * B + b]) == 0 ? 1u : 0u) << p;
        }
        const uint32_t tc = tcount ? (uint32_t)__builtin_amdgcn_readfirstlane((int)tcount[b]) : 0u;
        const uint32_t gid = (uint32_t)(first_env_id + (uint64_t)b);
        if (!((unsigned)sp < (unsigned)P && ((p0.alive >> (sp & 7)) & 1u) && (P == 1 || __popc(p0.alive) >= 2))) {   // skipped: zeros
            if (lane < 3) { visits[b * 3 + lane] = 0u; value[b * 3 + lane] = 0u; }
            if (lane == 0) { nodes[b] = 0u; best[b] = -1; }
            continue;
        }
        // ---- the root bitboard, lanes over words; the root node
        for (int w = lane; w < nwords; w += 64) root_bits[w] = tm_occ_run(board + b * NN + 32 * w, min(32, NN - 32 * w));
        if (lane == 0) { n_arr[0] = 0u; w_arr[0] = 0u; path[0] = 0; }
        if (lane < 3) child[lane] = 0;
        tm_wave_sync();
        int nn = 1;                                              // nodes so far
        for (int s = 0; s < S; ++s) {
            for (int w = lane; w < nwords; w += 64) work_bits[w] = root_bits[w];
            tm_wave_sync();
            TmPos<P> ps = p0;
            int v = 0, d = 0;
            bool closed, seat_alive;
            for (;;) {
                CRL_BOUNDS_LT(v, S + 1, 174);
                const uint32_t cu = lane < 3 ? child[v * 3 + lane] : 0u;
                CRL_BOUNDS_LT(cu, S + 1, 175);
                const unsigned long long fresh = __ballot(lane < 3 && cu == 0u);
                int e, u;
                if (fresh) {                                     // expand: the lowest action without a child
                    e = (int)__builtin_ctzll(fresh);
                    u = nn++;
                    CRL_BOUNDS_LT(u, S + 1, 176);
                    if (lane == 0) { child[v * 3 + e] = (uint16_t)u; n_arr[u] = 0u; w_arr[u] = 0u; }
                    if (lane < 3) child[u * 3 + lane] = 0;
                } else {                                         // select: lane a scores the child at action a
                    const uint32_t lgv = tm_lg(n_arr[v]);
                    uint32_t key = 0;
                    if (lane < 3) {
                        const uint32_t nu = n_arr[cu], wu = w_arr[cu];
                        const uint64_t exploit = tm_div((uint64_t)wu << 15, nu * (uint32_t)R);
                        const uint64_t X = tm_div((uint64_t)lgv << 24, nu);
                        const uint64_t score = exploit + (((uint64_t)cexp * tm_isqrt(X)) >> 8);   // < 2^26
                        key = (((uint32_t)score << 2) | (uint32_t)(3 - lane)) + 1u;               // ties: the lowest action
                    }
                    // the arg-max over the three lanes (every lane runs the reads: they sit outside the branch above)
                    const uint32_t k0 = (uint32_t)__builtin_amdgcn_readlane((int)key, 0), k1 = (uint32_t)__builtin_amdgcn_readlane((int)key, 1),
                                   k2 = (uint32_t)__builtin_amdgcn_readlane((int)key, 2);
                    const uint32_t top = max(k0, max(k1, k2));
                    e = 3 - (int)((top - 1u) & 3u);
                    const int c0 = __builtin_amdgcn_readlane((int)cu, 0), c1 = __builtin_amdgcn_readlane((int)cu, 1),
                              c2 = __builtin_amdgcn_readlane((int)cu, 2);
                    u = e == 0 ? c0 : e == 1 ? c1 : c2;
                }
                d += 1;
                CRL_BOUNDS_LT(d, S + 1, 177);
                if (lane == 0) path[d] = (uint16_t)u;
                // ---- the tree step at depth d - 1: the seat plays e, the others the model agent on the pre-step position
                int code[P];
                const uint32_t c = tc + (uint32_t)(d - 1);
                if constexpr (AVOID) {
                    tm_avoid_codes<P>(N, work, ps, gid, c, kTreeStep, seed_lo, seed_hi, thr, code);
                } else {
                    TmDraw dr = {};
                    tm_random_refill<P>(gid, c, kTreeStep, seed_lo, seed_hi, dr);
                    tm_random_codes<P>(c, dr, code);
                }
#pragma unroll
                for (int p = 0; p < P; ++p) code[p] = (p == sp) ? e + (e >> 1) : code[p];
                tm_step<P>(N, work, ps, code);
                seat_alive = (ps.alive >> sp) & 1u;
                closed = !seat_alive || __popc(ps.alive) <= 1;
                if (fresh || closed || d >= S) break;            // (d >= S: never, a path of d edges has d nodes below the root)
                v = u;
            }
            // ---- evaluate the leaf: its outcome when it is closed, else R playouts, lane r playout r
            uint32_t sum = closed ? (seat_alive ? 2u * (uint32_t)R : 0u) : 0u;      // half-points (wave-uniform)
            if (!closed) {
                tm_wave_sync();
                for (int r0 = 0; r0 < R; r0 += 64) {
                    const uint32_t r = (uint32_t)(r0 + lane);
                    const bool live = r < (uint32_t)R;
                    int hp = 0;
                    if (live) {
                        for (int w = 0; w < nwords; ++w) mine.bits[w * nslots + mine.slot] = work_bits[w];
                        TmPos<P> q = ps;
                        const uint32_t c2 = ((uint32_t)s << 16) | r;
                        uint32_t c = tc + (uint32_t)d;
                        int len = 0;
                        TmDraw dr = {};
                        for (;;) {
                            int code[P];
                            if constexpr (AVOID) {
                                tm_avoid_codes<P>(N, mine, q, gid, c, c2, seed_lo, seed_hi, thr, code);
                            } else {
                                if (len == 0 || (c & 7u) == 0u) tm_random_refill<P>(gid, c, c2, seed_lo, seed_hi, dr);
                                tm_random_codes<P>(c, dr, code);
                            }
                            tm_step<P>(N, mine, q, code);
                            len += 1;
                            const bool q_alive = (q.alive >> sp) & 1u;
                            if (__popc(q.alive) <= 1) { hp = q_alive ? 2 : 0; break; }
                            if (!q_alive) break;
                            if (len == max_steps) { hp = 1; break; }     // (max_steps = 0: no cap)
                            c += 1u;
                        }
                    }
                    sum += 2u * (uint32_t)__builtin_popcountll(__ballot(live && hp == 2)) +
                           (uint32_t)__builtin_popcountll(__ballot(live && hp == 1));
                }
            }
            // ---- back up: lane i adds to the node at depth i (distinct nodes: no atomics), 64 entries per pass
            tm_wave_sync();
            for (int i0 = 0; i0 <= d; i0 += 64) {
                const int i = i0 + lane;
                if (i <= d) {
                    const uint32_t node = path[i];
                    CRL_BOUNDS_LT(node, S + 1, 178);
                    n_arr[node] += 1u;
                    if (i > 0) w_arr[node] += sum;
                }
            }
            tm_wave_sync();
        }
        // ---- the root's children: visits, value, the most visited (then the larger w, then the lower action)
        const uint32_t cu = lane < 3 ? child[lane] : 0u;
        CRL_BOUNDS_LT(cu, S + 1, 179);
        const uint32_t vis = cu ? n_arr[cu] : 0u, val = cu ? w_arr[cu] : 0u;
        if (lane < 3) { visits[b * 3 + lane] = vis; value[b * 3 + lane] = val; }
        int pick = -1;
        uint32_t pick_n = 0u, pick_w = 0u;
#pragma unroll
        for (int a = 0; a < 3; ++a) {                            // (every lane runs the reads)
            const uint32_t ca = (uint32_t)__builtin_amdgcn_readlane((int)cu, a), na = (uint32_t)__builtin_amdgcn_readlane((int)vis, a),
                           wa = (uint32_t)__builtin_amdgcn_readlane((int)val, a);
            const bool better = ca != 0u && (pick < 0 || na > pick_n || (na == pick_n && wa > pick_w));
            pick = better ? a : pick;
            pick_n = better ? na : pick_n;
            pick_w = better ? wa : pick_w;
        }
        if (lane == 0) { nodes[b] = (uint32_t)nn; best[b] = pick; }
        tm_wave_sync();                                          // the next tree starts behind these reads
    }
}

// ------------------------------------------------------------------------------------------------ territory leaves
// crl_tron_mcts_territory: the same tree, the same descent, and a leaf valued by ONE Voronoi flood of
// its position instead of R playouts.  The flood is tron_territory.hip's register flood (terr_flood_rows there), restated
// here from the contract of crl_tron_territory: lane y is board row y, the row one 32- or 64-bit word, vertical neighbours
// by the two DPP wave shifts, frontiers and sums in registers, an empty ballot ends the loop.

template <int CTRL>
__device__ __forceinline__ uint32_t tm_dpp(const uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);   // (no source lane: 0)
}
template <int CTRL>
__device__ __forceinline__ uint64_t tm_dpp(const uint64_t v)
{
    return (uint64_t)tm_dpp<CTRL>((uint32_t)v) | ((uint64_t)tm_dpp<CTRL>((uint32_t)(v >> 32)) << 32);
}
constexpr int kTmDppWaveShl1 = 0x130;   // lane i reads lane i + 1
constexpr int kTmDppWaveShr1 = 0x138;   // lane i reads lane i - 1

__device__ __forceinline__ int tm_popc(const uint32_t v) { return __popc(v); }
__device__ __forceinline__ int tm_popc(const uint64_t v) { return __popcll(v); }

// 32 bits of the flat bitboard from bit `bit` on (any alignment): two dword reads and a funnel shift.  The second read is
// clamped onto the board's last word; it is only used where the run reaches into it.
__device__ __forceinline__ uint32_t tm_bits32(const uint32_t *bits, const int nwords, const int bit, const int code)
{
    const int i0 = bit >> 5, i1 = min(i0 + 1, nwords - 1);
    CRL_BOUNDS_LT(i0, nwords, code);
    CRL_BOUNDS_LT(i1, nwords, code + 1);
    (void)code;
    return (uint32_t)((((uint64_t)bits[i1] << 32) | (uint64_t)bits[i0]) >> (bit & 31));
}

// board row y (N <= 8 sizeof(W) cells from bit y * N on) of the flat bitboard, occupied cells set
template <typename W>
__device__ __forceinline__ W tm_row(const uint32_t *bits, const int nwords, const int N, const int y)
{
    const int bit = y * N;
    W row = (W)tm_bits32(bits, nwords, bit, 180);
    if constexpr (sizeof(W) == 8) row |= (W)tm_bits32(bits, nwords, bit + 32, 182) << 32;   // (N >= 33: bit + 32 < (y + 1) N <= N*N)
    return row;
}

// The leaf's areas: crl_tron_territory's definition with nobody forced on the position (work bitboard, ps).  Every lane of
// the wave runs this (the cross-lane reads need all 64); area[p] is the wave's total, alike in every lane.
template <int P, typename W>
__device__ __forceinline__ void tm_leaf_areas(const int N, const int NN, const int nwords, const int lane, const uint32_t *work_bits,
                                              const TmPos<P> &ps, int (&area)[P])
{
    const bool in_row = lane < N;
    const W rowmask = (W)(N >= (int)(8 * sizeof(W)) ? ~(W)0 : (((W)1 << N) - 1u));
    W free = in_row ? (W)~tm_row<W>(work_bits, nwords, N, in_row ? lane : 0) & rowmask : (W)0;
    W nw[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {                               // the first cells forward / right / left that lie in this row
        W bits = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int dd = (ps.d[p] + (a == 0 ? 0 : a == 1 ? 1 : 3)) & 3;
            const int nx = ps.x[p] + (dd == 1) - (dd == 3), ny = ps.y[p] + (dd == 2) - (dd == 0);
            const bool on = ((ps.alive >> p) & 1u) && (unsigned)nx < (unsigned)N && ny == lane;   // (ny == lane < N: on the board)
            bits |= on ? (W)1 << (nx & (int)(8 * sizeof(W) - 1)) : (W)0;
        }
        nw[p] = bits & free;
    }
    const W up_ok = (in_row && lane > 0) ? ~(W)0 : (W)0;         // takes from lane - 1: not the first row
    const W dn_ok = lane < N - 1 ? ~(W)0 : (W)0;                 // takes from lane + 1: not the last row (nor lane N's zeros)
    int mine[P];
#pragma unroll
    for (int p = 0; p < P; ++p) mine[p] = 0;
    for (int lvl = 0; lvl <= NN; ++lvl) {                        // (hard bound: a level with a new bit claims a cell)
        W once = 0, twice = 0;
#pragma unroll
        for (int p = 0; p < P; ++p) { twice |= once & nw[p]; once |= nw[p]; }
#pragma unroll
        for (int p = 0; p < P; ++p) mine[p] += tm_popc((W)(nw[p] & ~twice));
        free &= ~once;
        if (__ballot(once != 0) == 0ull) break;
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const W f = nw[p];
            nw[p] = ((W)(f << 1) | (W)(f >> 1) | (tm_dpp<kTmDppWaveShr1>(f) & up_ok) | (tm_dpp<kTmDppWaveShl1>(f) & dn_ok)) & free;
        }
    }
    // the sums over the wave, two 16-bit sums per shuffled word (an area is at most 64 * 64), a butterfly: every lane ends
    // with the totals
    constexpr int H = (P + 1) / 2;
    uint32_t v[H];
#pragma unroll
    for (int j = 0; j < H; ++j) v[j] = 0u;
#pragma unroll
    for (int p = 0; p < P; ++p) v[p >> 1] |= (uint32_t)mine[p] << ((p & 1) * 16);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
        for (int j = 0; j < H; ++j) v[j] += (uint32_t)__shfl_xor((int)v[j], off);
    }
#pragma unroll
    for (int p = 0; p < P; ++p) area[p] = __builtin_amdgcn_readfirstlane((int)((v[p >> 1] >> ((p & 1) * 16)) & 0xffffu));
}

template <int P, bool AVOID, typename W>
__global__ void __launch_bounds__(256)
tron_mcts_territory_kernel(const int N, const int NN, const uint32_t inv_n, const int64_t B, const uint32_t seed_lo,
                           const uint32_t seed_hi, const uint64_t first_env_id, const int8_t *__restrict__ board,
                           const int16_t *__restrict__ heads, const int8_t *__restrict__ dirs, const int8_t *__restrict__ deaths,
                           const uint32_t *__restrict__ tcount, const int8_t *__restrict__ seat_in, const int S, const int V,
                           const uint32_t cexp, const uint64_t thr, const int nwords, const uint32_t wave_words,
                           uint32_t *__restrict__ visits, uint32_t *__restrict__ value, uint32_t *__restrict__ nodes,
                           int32_t *__restrict__ best)
{
    // per wave: n[S + 1] | w[S + 1] | child uint16 [S + 1][3] | path uint16 [S + 1] | root[nwords] | work[nwords]
    extern __shared__ __attribute__((aligned(16))) uint32_t tm_lds[];
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), n_waves = (int)(blockDim.x >> 6);
    uint32_t *n_arr = tm_lds + (uint32_t)wave * wave_words, *w_arr = n_arr + (S + 1);
    uint16_t *child = reinterpret_cast<uint16_t *>(w_arr + (S + 1)), *path = child + 3 * (S + 1);
    uint32_t *root_bits = w_arr + 3 * (S + 1), *work_bits = root_bits + nwords;
    const TmBoard work = {work_bits, 1, 0, nwords};
    constexpr uint32_t kTreeStep = 0xFFFF0000u;                 // the third counter word of the tree steps' draws

    for (int64_t b = (int64_t)blockIdx.x * n_waves + wave; b < B; b += (int64_t)gridDim.x * n_waves) {
        // ---- the root position, alike in every lane
        const int sp = seat_in ? __builtin_amdgcn_readfirstlane((int)seat_in[b]) : 0;
        TmPos<P> p0;
        p0.alive = 0u;
#pragma unroll
        for (int p = 0; p < P; ++p) {
            p0.h[p] = min(max(__builtin_amdgcn_readfirstlane((int)heads[p * B + b]), 0), NN - 1);   // (a broken state: wrong results, no wild access)
            p0.y[p] = (int)__umulhi((uint32_t)p0.h[p], inv_n);
            p0.x[p] = p0.h[p] - p0.y[p] * N;
            p0.d[p] = __builtin_amdgcn_readfirstlane((int)dirs[p * B + b]) & 3;
            p0.alive |= (__builtin_amdgcn_readfirstlane((int)deaths[p * B + b]) == 0 ? 1u : 0u) << p;
        }
        const uint32_t tc = tcount ? (uint32_t)__builtin_amdgcn_readfirstlane((int)tcount[b]) : 0u;
        const uint32_t gid = (uint32_t)(first_env_id + (uint64_t)b);
        if (!((unsigned)sp < (unsigned)P && ((p0.alive >> (sp & 7)) & 1u) && (P == 1 || __popc(p0.alive) >= 2))) {   // skipped: zeros
            if (lane < 3) { visits[b * 3 + lane] = 0u; value[b * 3 + lane] = 0u; }
            if (lane == 0) { nodes[b] = 0u; best[b] = -1; }
            continue;
        }
        // ---- the root bitboard, lanes over words; the root node
        for (int w = lane; w < nwords; w += 64) root_bits[w] = tm_occ_run(board + b * NN + 32 * w, min(32, NN - 32 * w));
        if (lane == 0) { n_arr[0] = 0u; w_arr[0] = 0u; path[0] = 0; }
        if (lane < 3) child[lane] = 0;
        tm_wave_sync();
        int nn = 1;                                              // nodes so far
        for (int s = 0; s < S; ++s) {
            for (int w = lane; w < nwords; w += 64) work_bits[w] = root_bits[w];
            tm_wave_sync();
            TmPos<P> ps = p0;
            int v = 0, d = 0;
            bool closed, seat_alive;
            for (;;) {
                CRL_BOUNDS_LT(v, S + 1, 184);
                const uint32_t cu = lane < 3 ? child[v * 3 + lane] : 0u;
                CRL_BOUNDS_LT(cu, S + 1, 185);
                const unsigned long long fresh = __ballot(lane < 3 && cu == 0u);
                int e, u;
                if (fresh) {                                     // expand: the lowest action without a child
                    e = (int)__builtin_ctzll(fresh);
                    u = nn++;
                    CRL_BOUNDS_LT(u, S + 1, 186);
                    if (lane == 0) { child[v * 3 + e] = (uint16_t)u; n_arr[u] = 0u; w_arr[u] = 0u; }
                    if (lane < 3) child[u * 3 + lane] = 0;
                } else {                                         // select: lane a scores the child at action a
                    const uint32_t lgv = tm_lg(n_arr[v]);
                    uint32_t key = 0;
                    if (lane < 3) {
                        const uint32_t nu = n_arr[cu], wu = w_arr[cu];
                        const uint64_t exploit = tm_div((uint64_t)wu << 15, nu * (uint32_t)V);
                        const uint64_t X = tm_div((uint64_t)lgv << 24, nu);
                        const uint64_t score = exploit + (((uint64_t)cexp * tm_isqrt(X)) >> 8);   // < 2^26
                        key = (((uint32_t)score << 2) | (uint32_t)(3 - lane)) + 1u;               // ties: the lowest action
                    }
                    // the arg-max over the three lanes (every lane runs the reads: they sit outside the branch above)
                    const uint32_t k0 = (uint32_t)__builtin_amdgcn_readlane((int)key, 0), k1 = (uint32_t)__builtin_amdgcn_readlane((int)key, 1),
                                   k2 = (uint32_t)__builtin_amdgcn_readlane((int)key, 2);
                    const uint32_t top = max(k0, max(k1, k2));
                    e = 3 - (int)((top - 1u) & 3u);
                    const int c0 = __builtin_amdgcn_readlane((int)cu, 0), c1 = __builtin_amdgcn_readlane((int)cu, 1),
                              c2 = __builtin_amdgcn_readlane((int)cu, 2);
                    u = e == 0 ? c0 : e == 1 ? c1 : c2;
                }
                d += 1;
                CRL_BOUNDS_LT(d, S + 1, 187);
                if (lane == 0) path[d] = (uint16_t)u;
                // ---- the tree step at depth d - 1: the seat plays e, the others the model agent on the pre-step position
                int code[P];
                const uint32_t c = tc + (uint32_t)(d - 1);
                if constexpr (AVOID) {
                    tm_avoid_codes<P>(N, work, ps, gid, c, kTreeStep, seed_lo, seed_hi, thr, code);
                } else {
                    TmDraw dr = {};
                    tm_random_refill<P>(gid, c, kTreeStep, seed_lo, seed_hi, dr);
                    tm_random_codes<P>(c, dr, code);
                }
#pragma unroll
                for (int p = 0; p < P; ++p) code[p] = (p == sp) ? e + (e >> 1) : code[p];
                tm_step<P>(N, work, ps, code);
                seat_alive = (ps.alive >> sp) & 1u;
                closed = !seat_alive || __popc(ps.alive) <= 1;
                if (fresh || closed || d >= S) break;            // (d >= S: never, a path of d edges has d nodes below the root)
                v = u;
            }
            // ---- evaluate the leaf: its outcome when it is closed, else one flood of its position (no draw)
            uint32_t sum = seat_alive ? 2u * (uint32_t)V : 0u;   // half-points on the scale of V (wave-uniform)
            if (__builtin_amdgcn_readfirstlane((int)closed) == 0) {     // (alike in every lane: all 64 run the flood)
                tm_wave_sync();
                int area[P];
                tm_leaf_areas<P, W>(N, NN, nwords, lane, work_bits, ps, area);
                uint32_t a_s = 0u, a_o = 0u;
#pragma unroll
                for (int p = 0; p < P; ++p) {                    // (dead players hold 0)
                    a_s = p == sp ? (uint32_t)area[p] : a_s;
                    a_o = p == sp ? a_o : max(a_o, (uint32_t)area[p]);
                }
                const uint32_t den = a_s + a_o;
                sum = den == 0u ? (uint32_t)V : (uint32_t)tm_div((uint64_t)(2u * (uint32_t)V * a_s), den);
            }
            // ---- back up: lane i adds to the node at depth i (distinct nodes: no atomics), 64 entries per pass
            tm_wave_sync();
            for (int i0 = 0; i0 <= d; i0 += 64) {
                const int i = i0 + lane;
                if (i <= d) {
                    const uint32_t node = path[i];
                    CRL_BOUNDS_LT(node, S + 1, 188);
                    n_arr[node] += 1u;
                    if (i > 0) w_arr[node] += sum;
                }
            }
            tm_wave_sync();
        }
        // ---- the root's children: visits, value, the most visited (then the larger w, then the lower action)
        const uint32_t cu = lane < 3 ? child[lane] : 0u;
        CRL_BOUNDS_LT(cu, S + 1, 189);
        const uint32_t vis = cu ? n_arr[cu] : 0u, val = cu ? w_arr[cu] : 0u;
        if (lane < 3) { visits[b * 3 + lane] = vis; value[b * 3 + lane] = val; }
        int pick = -1;
        uint32_t pick_n = 0u, pick_w = 0u;
#pragma unroll
        for (int a = 0; a < 3; ++a) {                            // (every lane runs the reads)
            const uint32_t ca = (uint32_t)__builtin_amdgcn_readlane((int)cu, a), na = (uint32_t)__builtin_amdgcn_readlane((int)vis, a),
                           wa = (uint32_t)__builtin_amdgcn_readlane((int)val, a);
            const bool better = ca != 0u && (pick < 0 || na > pick_n || (na == pick_n && wa > pick_w));
            pick = better ? a : pick;
            pick_n = better ? na : pick_n;
            pick_w = better ? wa : pick_w;
        }
        if (lane == 0) { nodes[b] = (uint32_t)nn; best[b] = pick; }
        tm_wave_sync();                                          // the next tree starts behind these reads
    }
}

// one wave's slice of LDS: n[S + 1] | w[S + 1] | child uint16 [S + 1][3] | path uint16 [S + 1] | root[nwords] | work[nwords],
// 4 (S + 1) + 2 nwords dwords from `base` on
struct TmTree {
    uint32_t *n_arr, *w_arr;
    uint16_t *child, *path;
    uint32_t *root_bits, *work_bits;
};

__device__ __forceinline__ TmTree tm_tree_at(uint32_t *base, const int S, const int nwords)
{
    TmTree t;
    t.n_arr = base;
    t.w_arr = t.n_arr + (S + 1);
    t.child = reinterpret_cast<uint16_t *>(t.w_arr + (S + 1));
    t.path = t.child + 3 * (S + 1);
    t.root_bits = t.w_arr + 3 * (S + 1);
    t.work_bits = t.root_bits + nwords;
    return t;
}

// the root position of game b, alike in every lane
template <int P>
__device__ __forceinline__ TmPos<P> tm_root_pos(const int N, const int NN, const uint32_t inv_n, const int64_t B, const int64_t b,
                                                const int16_t *__restrict__ heads, const int8_t *__restrict__ dirs,
                                                const int8_t *__restrict__ deaths)
{
    TmPos<P> p0;
    p0.alive = 0u;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        p0.h[p] = min(max(__builtin_amdgcn_readfirstlane((int)heads[p * B + b]), 0), NN - 1);   // (a broken state: wrong results, no wild access)
        p0.y[p] = (int)__umulhi((uint32_t)p0.h[p], inv_n);
        p0.x[p] = p0.h[p] - p0.y[p] * N;
        p0.d[p] = __builtin_amdgcn_readfirstlane((int)dirs[p * B + b]) & 3;
        p0.alive |= (__builtin_amdgcn_readfirstlane((int)deaths[p * B + b]) == 0 ? 1u : 0u) << p;
    }
    return p0;
}

// The search of crl_tron_mcts_territory for the live seat sp of ONE position, by one wave in its own slice of LDS, for
// tron_sample_mcts_territory_kernel (below): the body of tron_mcts_territory_kernel (above) from the root bitboard (built from
// `cells`, the position's N*N board bytes) to the pick, statement for statement, with the same CRL_BOUNDS_LT sites.  It is a
// second copy: with both kernels on this function crl_tron_mcts_territory measured 1.0-2.2 % slower than before (DESIGN.md
// section 4.5g), so that kernel stays as it was; a change to the search goes into both, and the differential test of the two
// entries (tests/test_gpu_tron_mcts_agent.py) holds them to each other.  Returns best (never -1: S >= 1); vis / val are the
// root's child at action `lane` in lanes 0..2, nn the node count.  The caller has checked the skipped-position rule and puts
// a tm_wave_sync between this and the next use of the slice.
template <int P, bool AVOID, typename W>
__device__ __forceinline__ int tm_territory_search(const int N, const int NN, const int nwords, const int lane,
                                                   const int8_t *__restrict__ cells, const TmPos<P> &p0, const int sp,
                                                   const uint32_t tc, const uint32_t gid, const uint32_t seed_lo,
                                                   const uint32_t seed_hi, const int S, const int V, const uint32_t cexp,
                                                   const uint64_t thr, const TmTree &t, uint32_t &vis, uint32_t &val, int &nn)
{
    uint32_t *const n_arr = t.n_arr, *const w_arr = t.w_arr, *const root_bits = t.root_bits, *const work_bits = t.work_bits;
    uint16_t *const child = t.child, *const path = t.path;
    const TmBoard work = {work_bits, 1, 0, nwords};
    constexpr uint32_t kTreeStep = 0xFFFF0000u;                 // the third counter word of the tree steps' draws
    // ---- the root bitboard, lanes over words; the root node
    for (int w = lane; w < nwords; w += 64) root_bits[w] = tm_occ_run(cells + 32 * w, min(32, NN - 32 * w));
    if (lane == 0) { n_arr[0] = 0u; w_arr[0] = 0u; path[0] = 0; }
    if (lane < 3) child[lane] = 0;
    tm_wave_sync();
    nn = 1;                                                  // nodes so far
    for (int s = 0; s < S; ++s) {
        for (int w = lane; w < nwords; w += 64) work_bits[w] = root_bits[w];
        tm_wave_sync();
        TmPos<P> ps = p0;
        int v = 0, d = 0;
        bool closed, seat_alive;
        for (;;) {
            CRL_BOUNDS_LT(v, S + 1, 184);
            const uint32_t cu = lane < 3 ? child[v * 3 + lane] : 0u;
            CRL_BOUNDS_LT(cu, S + 1, 185);
            const unsigned long long fresh = __ballot(lane < 3 && cu == 0u);
            int e, u;
            if (fresh) {                                     // expand: the lowest action without a child
                e = (int)__builtin_ctzll(fresh);
                u = nn++;
                CRL_BOUNDS_LT(u, S + 1, 186);
                if (lane == 0) { child[v * 3 + e] = (uint16_t)u; n_arr[u] = 0u; w_arr[u] = 0u; }
                if (lane < 3) child[u * 3 + lane] = 0;
            } else {                                         // select: lane a scores the child at action a
                const uint32_t lgv = tm_lg(n_arr[v]);
                uint32_t key = 0;
                if (lane < 3) {
                    const uint32_t nu = n_arr[cu], wu = w_arr[cu];
                    const uint64_t exploit = tm_div((uint64_t)wu << 15, nu * (uint32_t)V);
                    const uint64_t X = tm_div((uint64_t)lgv << 24, nu);
                    const uint64_t score = exploit + (((uint64_t)cexp * tm_isqrt(X)) >> 8);   // < 2^26
                    key = (((uint32_t)score << 2) | (uint32_t)(3 - lane)) + 1u;               // ties: the lowest action
                }
                // the arg-max over the three lanes (every lane runs the reads: they sit outside the branch above)
                const uint32_t k0 = (uint32_t)__builtin_amdgcn_readlane((int)key, 0), k1 = (uint32_t)__builtin_amdgcn_readlane((int)key, 1),
                               k2 = (uint32_t)__builtin_amdgcn_readlane((int)key, 2);
                const uint32_t top = max(k0, max(k1, k2));
                e = 3 - (int)((top - 1u) & 3u);
                const int c0 = __builtin_amdgcn_readlane((int)cu, 0), c1 = __builtin_amdgcn_readlane((int)cu, 1),
                          c2 = __builtin_amdgcn_readlane((int)cu, 2);
                u = e == 0 ? c0 : e == 1 ? c1 : c2;
            }
            d += 1;
            CRL_BOUNDS_LT(d, S + 1, 187);
            if (lane == 0) path[d] = (uint16_t)u;
            // ---- the tree step at depth d - 1: the seat plays e, the others the model agent on the pre-step position
            int code[P];
            const uint32_t c = tc + (uint32_t)(d - 1);
            if constexpr (AVOID) {
                tm_avoid_codes<P>(N, work, ps, gid, c, kTreeStep, seed_lo, seed_hi, thr, code);
            } else {
                TmDraw dr = {};
                tm_random_refill<P>(gid, c, kTreeStep, seed_lo, seed_hi, dr);
                tm_random_codes<P>(c, dr, code);
            }
#pragma unroll
            for (int p = 0; p < P; ++p) code[p] = (p == sp) ? e + (e >> 1) : code[p];
            tm_step<P>(N, work, ps, code);
            seat_alive = (ps.alive >> sp) & 1u;
            closed = !seat_alive || __popc(ps.alive) <= 1;
            if (fresh || closed || d >= S) break;            // (d >= S: never, a path of d edges has d nodes below the root)
            v = u;
        }
        // ---- evaluate the leaf: its outcome when it is closed, else one flood of its position (no draw)
        uint32_t sum = seat_alive ? 2u * (uint32_t)V : 0u;   // half-points on the scale of V (wave-uniform)
        if (__builtin_amdgcn_readfirstlane((int)closed) == 0) {     // (alike in every lane: all 64 run the flood)
            tm_wave_sync();
            int area[P];
            tm_leaf_areas<P, W>(N, NN, nwords, lane, work_bits, ps, area);
            uint32_t a_s = 0u, a_o = 0u;
#pragma unroll
            for (int p = 0; p < P; ++p) {                    // (dead players hold 0)
                a_s = p == sp ? (uint32_t)area[p] : a_s;
                a_o = p == sp ? a_o : max(a_o, (uint32_t)area[p]);
            }
            const uint32_t den = a_s + a_o;
            sum = den == 0u ? (uint32_t)V : (uint32_t)tm_div((uint64_t)(2u * (uint32_t)V * a_s), den);
        }
        // ---- back up: lane i adds to the node at depth i (distinct nodes: no atomics), 64 entries per pass
        tm_wave_sync();
        for (int i0 = 0; i0 <= d; i0 += 64) {
            const int i = i0 + lane;
            if (i <= d) {
                const uint32_t node = path[i];
                CRL_BOUNDS_LT(node, S + 1, 188);
                n_arr[node] += 1u;
                if (i > 0) w_arr[node] += sum;
            }
        }
        tm_wave_sync();
    }
    // ---- the root's children: visits, value, the most visited (then the larger w, then the lower action)
    const uint32_t cu = lane < 3 ? child[lane] : 0u;
    CRL_BOUNDS_LT(cu, S + 1, 189);
    vis = cu ? n_arr[cu] : 0u;
    val = cu ? w_arr[cu] : 0u;
    int pick = -1;
    uint32_t pick_n = 0u, pick_w = 0u;
#pragma unroll
    for (int a = 0; a < 3; ++a) {                            // (every lane runs the reads)
        const uint32_t ca = (uint32_t)__builtin_amdgcn_readlane((int)cu, a), na = (uint32_t)__builtin_amdgcn_readlane((int)vis, a),
                       wa = (uint32_t)__builtin_amdgcn_readlane((int)val, a);
        const bool better = ca != 0u && (pick < 0 || na > pick_n || (na == pick_n && wa > pick_w));
        pick = better ? a : pick;
        pick_n = better ? na : pick_n;
        pick_w = better ? wa : pick_w;
    }
    return pick;
}

// the k-th set bit of mask (k < popcount(mask))
__device__ __forceinline__ int tm_kth_bit(uint32_t mask, int k)
{
    while (k-- > 0) mask &= mask - 1u;
    return (int)__builtin_ctz(mask);
}

// crl_tron_sample_mcts_territory: the search above as a seated agent.  One workgroup holds one game,
// wave j is the j-th player of the mask (m = popcount(pmask) waves, 64 m threads) with a slice of LDS of its own, so the m
// searches of a game run side by side and share nothing.  The games are walked in a grid-stride loop that is uniform over the
// workgroup: every wave, whether it searches, is noisy or sits on a dead seat, makes the same trips and meets the ONE
// workgroup barrier of a trip -- every wave has read the game's counter in front of it, wave 0 advances the counter behind it.
template <int P, bool AVOID, typename W>
__global__ void __launch_bounds__(512)
tron_sample_mcts_territory_kernel(const int N, const int NN, const uint32_t inv_n, const int64_t B, const uint32_t seed_lo,
                                  const uint32_t seed_hi, const uint64_t first_env_id, const int8_t *__restrict__ board,
                                  const int16_t *__restrict__ heads, const int8_t *__restrict__ dirs,
                                  const int8_t *__restrict__ deaths, uint32_t *tcount, const int advance, const uint64_t noise_thr,
                                  const uint32_t pmask, const int S, const int V, const uint32_t cexp, const uint64_t thr,
                                  const int nwords, const uint32_t wave_words, int8_t *__restrict__ actions)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t tm_lds[];
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    CRL_BOUNDS_LT(wave, __popc(pmask), 190);
    CRL_BOUNDS_LT((uint32_t)wave * wave_words + wave_words - 1u, (uint32_t)(blockDim.x >> 6) * wave_words, 191);
    const int sp = tm_kth_bit(pmask, wave);                     // this wave's seat
    const TmTree tree = tm_tree_at(tm_lds + (uint32_t)wave * wave_words, S, nwords);

    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {       // (alike in every wave of the workgroup)
        const TmPos<P> p0 = tm_root_pos<P>(N, NN, inv_n, B, b, heads, dirs, deaths);
        const uint32_t tc = (uint32_t)__builtin_amdgcn_readfirstlane((int)tcount[b]);
        const uint32_t gid = (uint32_t)(first_env_id + (uint64_t)b);
        __syncthreads();                                         // every wave holds the counter: wave 0 may advance it
        if (advance && threadIdx.x == 0u) tcount[b] = tc + 1u;
        int a = 0;                                               // dead players: 0
        if ((p0.alive >> sp) & 1u) {
            const philox_out wv = philox4x32_10(gid, tc, (uint32_t)sp, CRL_TAG_TRON_TERRITORY, seed_lo, seed_hi);   // (wave-uniform)
            if ((uint64_t)wv.w[0] < noise_thr) {
                a = (int)__umulhi(wv.w[1], 3u);
            } else if (P == 1 || __popc(p0.alive) >= 2) {        // (else crl_tron_mcts_territory skips: best -1 plays 0)
                uint32_t vis, val;
                int nn;
                a = tm_territory_search<P, AVOID, W>(N, NN, nwords, lane, board + b * NN, p0, sp, tc, gid, seed_lo, seed_hi, S, V, cexp,
                                                     thr, tree, vis, val, nn);
                tm_wave_sync();                                  // the next tree starts behind the pick's reads
            }
        }
        if (lane == 0) actions[(int64_t)sp * B + b] = (int8_t)(a == 2 ? -1 : a);
    }
}

// S_max of crl_tron_mcts (include/colosseum_hip.h): the tree, the path and the 66 bitboards of one wave within 64 KB, and
// s < 4095 (its counter word); below 1 on boards of 90x90 and more
constexpr uint32_t kTmLds = 65536u;
int tron_mcts_max_simulations(const int N)
{
    const int nwords = (N * N + 31) >> 5;
    const int s = ((int)kTmLds - 264 * nwords) / 16 - 1;        // (C's division: a negative numerator stays below 1)
    return s < 4095 ? s : 4095;
}

// S_agent of crl_tron_sample_mcts_territory: m waves of crl_tron_mcts_territory's per-wave LDS (16 (S + 1) + 8 nwords bytes)
// in one workgroup's 64 KB, and no more than S_max above
int tron_mcts_agent_max_simulations(const int N, const int m)
{
    const int nwords = (N * N + 31) >> 5;
    const int s = ((int)kTmLds / m - 8 * nwords) / 16 - 1, s_max = tron_mcts_max_simulations(N);
    return s < s_max ? s : s_max;
}

} // namespace

int crl_tron_mcts_bounds(unsigned int *out4)
{
    CRL_BOUNDS_READBACK(out4);
    return CRL_OK;
}

int crl_tron_mcts_max_simulations(const crl_ctx *ctx)
{
    CRL_REQUIRE(ctx != nullptr && ctx->game == CRL_GAME_TRON, "crl_tron_mcts_max_simulations: ctx is not a tron context");
    const int s_max = tron_mcts_max_simulations(ctx->tron.N);
    if (s_max < 1) {
        crl_set_error("crl_tron_mcts_max_simulations: a %dx%d board leaves no room for a tree in LDS", ctx->tron.N, ctx->tron.N);
        return CRL_EUNSUPPORTED;
    }
    return s_max;
}

int crl_tron_mcts(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id,
                  const int8_t *board, const int16_t *heads, const int8_t *dirs, const int8_t *deaths,
                  const uint32_t *tcount, const int8_t *seat, int S, int R, uint32_t cexp, double noise, int max_steps,
                  uint32_t *visits, uint32_t *value, uint32_t *nodes, int32_t *best, uint32_t flags, void *stream)
{
    TRON_CTX_CHECK("crl_tron_mcts");
    CRL_REQUIRE(board && heads && dirs && deaths, "crl_tron_mcts: NULL state pointer");
    CRL_REQUIRE(visits && value && nodes && best, "crl_tron_mcts: NULL output pointer");
    const crl_tron_cfg &cfg = ctx->tron;
    const int s_max = tron_mcts_max_simulations(cfg.N);
    if (s_max < 1) {
        crl_set_error("crl_tron_mcts: a %dx%d board leaves no room for a tree in LDS", cfg.N, cfg.N);
        return CRL_EUNSUPPORTED;
    }
    CRL_REQUIRE(S >= 1 && S <= s_max, "crl_tron_mcts: S=%d out of range 1..%d (a %dx%d board)", S, s_max, cfg.N, cfg.N);
    CRL_REQUIRE(R >= 1 && R <= 1024, "crl_tron_mcts: R=%d out of range 1..1024", R);
    CRL_REQUIRE(cexp <= 65535u, "crl_tron_mcts: cexp=%u out of range 0..65535", cexp);
    CRL_REQUIRE(noise >= 0.0 && noise <= 1.0, "crl_tron_mcts: noise=%g not in [0, 1]", noise);
    CRL_REQUIRE(max_steps >= 0 && max_steps <= 65535, "crl_tron_mcts: max_steps=%d out of range 0..65535", max_steps);
    CRL_REQUIRE((flags & ~CRL_PLAYOUT_AVOID) == 0u, "crl_tron_mcts: unknown flags 0x%x", flags);
    // one to four waves per workgroup, as many as fit in 64 KB; a grid-stride loop past 2^20 workgroups
    const int NN = cfg.N * cfg.N, nwords = (NN + 31) >> 5;
    const uint32_t wave_bytes = 16u * (uint32_t)(S + 1) + 264u * (uint32_t)nwords;
    uint32_t waves = kTmLds / wave_bytes;
    waves = waves > 4u ? 4u : waves;
    waves = (int64_t)waves > B ? (uint32_t)B : waves;
    const uint64_t want = ((uint64_t)B + waves - 1u) / waves;
    const unsigned blocks = (unsigned)(want < (1u << 20) ? want : (1u << 20));
    const uint32_t wave_words = 4u * (uint32_t)(S + 1) + 2u * (uint32_t)nwords;
    const uint32_t inv_n = (uint32_t)(0x100000000ull / (uint32_t)cfg.N) + 1u;   // y = umulhi(h, inv_n) is exact for h < N*N <= 2^15
    const uint64_t thr = crl_noise_threshold(noise);
    hipStream_t st = (hipStream_t)stream;
#define TRON_MCTS_LAUNCH(AV_)                                                                                              \
    hipLaunchKernelGGL((tron_mcts_kernel<PP, AV_>), dim3(blocks), dim3(64u * waves), (size_t)waves * wave_bytes, st, cfg.N, NN, \
                       inv_n, B, (uint32_t)seed, (uint32_t)(seed >> 32), first_env_id, board, heads, dirs, deaths, tcount, seat, \
                       S, R, cexp, thr, max_steps, nwords, wave_words, visits, value, nodes, best)
    if (flags & CRL_PLAYOUT_AVOID) {
        TRON_DISPATCH_P(cfg.P, TRON_MCTS_LAUNCH(true));
    } else {
        TRON_DISPATCH_P(cfg.P, TRON_MCTS_LAUNCH(false));
    }
#undef TRON_MCTS_LAUNCH
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

int crl_tron_mcts_territory(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id,
                            const int8_t *board, const int16_t *heads, const int8_t *dirs, const int8_t *deaths,
                            const uint32_t *tcount, const int8_t *seat, int S, int V, uint32_t cexp, double noise,
                            uint32_t *visits, uint32_t *value, uint32_t *nodes, int32_t *best, uint32_t flags, void *stream)
{
    TRON_CTX_CHECK("crl_tron_mcts_territory");
    CRL_REQUIRE(board && heads && dirs && deaths, "crl_tron_mcts_territory: NULL state pointer");
    CRL_REQUIRE(visits && value && nodes && best, "crl_tron_mcts_territory: NULL output pointer");
    const crl_tron_cfg &cfg = ctx->tron;
    if (cfg.N > 64) {                                            // the flood is one lane per board row
        crl_set_error("crl_tron_mcts_territory: a %dx%d board is wider than 64, the widest the in-wave flood takes", cfg.N, cfg.N);
        return CRL_EUNSUPPORTED;
    }
    const int s_max = tron_mcts_max_simulations(cfg.N);         // crl_tron_mcts's, so that the two searches' trees compare
    CRL_REQUIRE(S >= 1 && S <= s_max, "crl_tron_mcts_territory: S=%d out of range 1..%d (a %dx%d board)", S, s_max, cfg.N, cfg.N);
    CRL_REQUIRE(V >= 1 && V <= 1024, "crl_tron_mcts_territory: V=%d out of range 1..1024", V);
    CRL_REQUIRE(cexp <= 65535u, "crl_tron_mcts_territory: cexp=%u out of range 0..65535", cexp);
    CRL_REQUIRE(noise >= 0.0 && noise <= 1.0, "crl_tron_mcts_territory: noise=%g not in [0, 1]", noise);
    CRL_REQUIRE((flags & ~CRL_PLAYOUT_AVOID) == 0u, "crl_tron_mcts_territory: unknown flags 0x%x", flags);
    // one to four waves per workgroup, as many as fit in 64 KB (four up to S = 959 on 64x64, more on smaller boards); a
    // grid-stride loop past 2^20 workgroups
    const int NN = cfg.N * cfg.N, nwords = (NN + 31) >> 5;
    const uint32_t wave_bytes = 16u * (uint32_t)(S + 1) + 8u * (uint32_t)nwords;
    uint32_t waves = kTmLds / wave_bytes;
    waves = waves > 4u ? 4u : waves;
    waves = (int64_t)waves > B ? (uint32_t)B : waves;
    const uint64_t want = ((uint64_t)B + waves - 1u) / waves;
    const unsigned blocks = (unsigned)(want < (1u << 20) ? want : (1u << 20));
    const uint32_t wave_words = 4u * (uint32_t)(S + 1) + 2u * (uint32_t)nwords;
    const uint32_t inv_n = (uint32_t)(0x100000000ull / (uint32_t)cfg.N) + 1u;   // y = umulhi(h, inv_n) is exact for h < N*N <= 2^15
    const uint64_t thr = crl_noise_threshold(noise);
    hipStream_t st = (hipStream_t)stream;
#define TRON_MCTS_TERR_LAUNCH(AV_, W_)                                                                                      \
    hipLaunchKernelGGL((tron_mcts_territory_kernel<PP, AV_, W_>), dim3(blocks), dim3(64u * waves), (size_t)waves * wave_bytes, st, \
                       cfg.N, NN, inv_n, B, (uint32_t)seed, (uint32_t)(seed >> 32), first_env_id, board, heads, dirs, deaths,   \
                       tcount, seat, S, V, cexp, thr, nwords, wave_words, visits, value, nodes, best)
    if (flags & CRL_PLAYOUT_AVOID) {
        TRON_DISPATCH_P(cfg.P, { if (cfg.N <= 32) TRON_MCTS_TERR_LAUNCH(true, uint32_t); else TRON_MCTS_TERR_LAUNCH(true, uint64_t); });
    } else {
        TRON_DISPATCH_P(cfg.P, { if (cfg.N <= 32) TRON_MCTS_TERR_LAUNCH(false, uint32_t); else TRON_MCTS_TERR_LAUNCH(false, uint64_t); });
    }
#undef TRON_MCTS_TERR_LAUNCH
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

int crl_tron_sample_mcts_territory_max_simulations(const crl_ctx *ctx, uint32_t player_mask)
{
    CRL_REQUIRE(ctx != nullptr && ctx->game == CRL_GAME_TRON, "crl_tron_sample_mcts_territory_max_simulations: ctx is not a tron context");
    const crl_tron_cfg &cfg = ctx->tron;
    CRL_REQUIRE(player_mask != 0u, "crl_tron_sample_mcts_territory_max_simulations: player_mask is empty");
    CRL_REQUIRE((player_mask >> cfg.P) == 0u, "crl_tron_sample_mcts_territory_max_simulations: player_mask 0x%x names players beyond P=%d",
                player_mask, cfg.P);
    if (cfg.N > 64) {
        crl_set_error("crl_tron_sample_mcts_territory_max_simulations: a %dx%d board is wider than 64, the widest the in-wave flood takes",
                      cfg.N, cfg.N);
        return CRL_EUNSUPPORTED;
    }
    return tron_mcts_agent_max_simulations(cfg.N, __builtin_popcount(player_mask));
}

int crl_tron_sample_mcts_territory(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, uint32_t *tcount, int advance,
                                   double noise, uint32_t player_mask, const int8_t *board, const int16_t *heads, const int8_t *dirs,
                                   const int8_t *deaths, int S, int V, uint32_t cexp, double model_noise, uint32_t flags,
                                   int8_t *actions, void *stream)
{
    TRON_CTX_CHECK("crl_tron_sample_mcts_territory");
    CRL_REQUIRE(tcount && actions, "crl_tron_sample_mcts_territory: NULL tcount / actions pointer");
    CRL_REQUIRE(board && heads && dirs && deaths, "crl_tron_sample_mcts_territory: NULL state pointer");
    const crl_tron_cfg &cfg = ctx->tron;
    CRL_REQUIRE(player_mask != 0u, "crl_tron_sample_mcts_territory: player_mask is empty");
    CRL_REQUIRE((player_mask >> cfg.P) == 0u, "crl_tron_sample_mcts_territory: player_mask 0x%x names players beyond P=%d", player_mask,
                cfg.P);
    if (cfg.N > 64) {                                            // the flood is one lane per board row
        crl_set_error("crl_tron_sample_mcts_territory: a %dx%d board is wider than 64, the widest the in-wave flood takes", cfg.N, cfg.N);
        return CRL_EUNSUPPORTED;
    }
    CRL_REQUIRE(noise >= 0.0 && noise <= 1.0, "crl_tron_sample_mcts_territory: noise=%g not in [0, 1]", noise);
    CRL_REQUIRE(model_noise >= 0.0 && model_noise <= 1.0, "crl_tron_sample_mcts_territory: model_noise=%g not in [0, 1]", model_noise);
    const uint32_t m = (uint32_t)__builtin_popcount(player_mask);
    const int s_agent = tron_mcts_agent_max_simulations(cfg.N, (int)m);
    CRL_REQUIRE(S >= 1 && S <= s_agent, "crl_tron_sample_mcts_territory: S=%d out of range 1..%d (a %dx%d board, %u players in the mask)",
                S, s_agent, cfg.N, cfg.N, m);
    CRL_REQUIRE(V >= 1 && V <= 1024, "crl_tron_sample_mcts_territory: V=%d out of range 1..1024", V);
    CRL_REQUIRE(cexp <= 65535u, "crl_tron_sample_mcts_territory: cexp=%u out of range 0..65535", cexp);
    CRL_REQUIRE((flags & ~CRL_PLAYOUT_AVOID) == 0u, "crl_tron_sample_mcts_territory: unknown flags 0x%x", flags);
    // one workgroup per game, one wave per masked player, each with crl_tron_mcts_territory's per-wave LDS (m of them fit 64 KB:
    // that is S_agent); a grid-stride loop past 2^20 workgroups
    const int NN = cfg.N * cfg.N, nwords = (NN + 31) >> 5;
    const uint32_t wave_bytes = 16u * (uint32_t)(S + 1) + 8u * (uint32_t)nwords;
    const unsigned blocks = (unsigned)(B < ((int64_t)1 << 20) ? B : ((int64_t)1 << 20));
    const uint32_t wave_words = 4u * (uint32_t)(S + 1) + 2u * (uint32_t)nwords;
    const uint32_t inv_n = (uint32_t)(0x100000000ull / (uint32_t)cfg.N) + 1u;   // y = umulhi(h, inv_n) is exact for h < N*N <= 2^15
    const uint64_t noise_thr = crl_noise_threshold(noise), thr = crl_noise_threshold(model_noise);
    hipStream_t st = (hipStream_t)stream;
#define TRON_MCTS_AGENT_LAUNCH(AV_, W_)                                                                                     \
    hipLaunchKernelGGL((tron_sample_mcts_territory_kernel<PP, AV_, W_>), dim3(blocks), dim3(64u * m), (size_t)m * wave_bytes, st, \
                       cfg.N, NN, inv_n, B, (uint32_t)seed, (uint32_t)(seed >> 32), first_env_id, board, heads, dirs, deaths,   \
                       tcount, advance, noise_thr, player_mask, S, V, cexp, thr, nwords, wave_words, actions)
    if (flags & CRL_PLAYOUT_AVOID) {
        TRON_DISPATCH_P(cfg.P, { if (cfg.N <= 32) TRON_MCTS_AGENT_LAUNCH(true, uint32_t); else TRON_MCTS_AGENT_LAUNCH(true, uint64_t); });
    } else {
        TRON_DISPATCH_P(cfg.P, { if (cfg.N <= 32) TRON_MCTS_AGENT_LAUNCH(false, uint32_t); else TRON_MCTS_AGENT_LAUNCH(false, uint64_t); });
    }
#undef TRON_MCTS_AGENT_LAUNCH
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}
