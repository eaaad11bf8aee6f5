// tron_puct.hip -- tree search valued by the caller's network for one seat of Tron (crl_tron_puct_*; the contract is in
// include/colosseum_hip.h), gfx950, wave64.
//
// The trees live in the caller's buffer in HBM between the launches, one wave per tree in every kernel.  As in crl_tron_mcts
// the tree branches on the seat's three actions only and every other player is part of the transition, so a node holds no
// position: `select` copies the root board from the tree into a byte board in LDS and replays the edges on it.  A tree of
// N = S_cap + 1 nodes on a board of NN cells (NNp = NN rounded up to 16) is, in bytes:
//   [0, 64)        16 header words: node count (0 = a skipped tree), simulation count, path length (0 = no path outstanding),
//                  leaf word (kind | seat alive << 8), seat, tcount, g, seed lo, seed hi, model (1 = avoid), the noise
//                  threshold lo, hi, four spare words
//   [64, 96)       the root's 8 player words: head | dir << 16 | (deaths & 255) << 24
//   [96, 96 + NNp) the root board bytes, the padding zero
//   then           n uint32 [N], w uint32 [N], prior uint16 [N][3], child uint16 [N][3] (0 = none), path uint16 [N]
// rounded up to 16 bytes.
// "Expanded" has no bit of its own: a descent only ever stands on the root or on a node it reached by a step that left it
// open, and such a node has priors exactly when a backup has passed through it, which is n > 0 (ttt_puct.hip's rule).
// The model draws and the step are restated here on a BYTE board (tron_mcts.hip restates them on a bitboard, tron.hip holds
// the originals): the step needs the owners, because the leaf goes out as a position with killer ids.
// The descent is wave-uniform: every lane holds the same player vectors, reads the LDS board at the same address and
// rewrites it with the same byte; what the loop branches on goes through v_readfirstlane.  Lanes hand values to each other
// through LDS only at the copy-in (lanes over 16-byte chunks) and the stream-out, across tp_wave_sync.
// Every index read out of the tree or the board is clamped before it addresses anything: a buffer that was never given to
// crl_tron_puct_begin cannot make a kernel write outside it.
#include "crl_common.hpp"

namespace {

constexpr int TP_H_NODES = 0, TP_H_SIMS = 1, TP_H_PATH = 2, TP_H_LEAF = 3, TP_H_SEAT = 4, TP_H_TCOUNT = 5, TP_H_GID = 6,
              TP_H_SEED_LO = 7, TP_H_SEED_HI = 8, TP_H_MODEL = 9, TP_H_THR_LO = 10, TP_H_THR_HI = 11;
constexpr int TP_HDR_BYTES = 64, TP_PLAYER_BYTES = 4 * CRL_TRON_MAX_P, TP_FIXED_BYTES = TP_HDR_BYTES + TP_PLAYER_BYTES;
constexpr uint32_t TP_PENDING = 1u, TP_TERMINAL = 2u;
constexpr int TP_MAX_S = 4095;
constexpr uint32_t TP_LDS = 65536u;
constexpr uint32_t TP_TREE_STEP = 0xFFFF0000u;                  // the third counter word of the tree steps' draws
static_assert(TP_FIXED_BYTES % 16 == 0 && CRL_TRON_MAX_P == 8, "a tree's fixed part");

__host__ __device__ inline uint32_t tp_board_bytes(const int NN) { return ((uint32_t)NN + 15u) & ~15u; }

// one wave's LDS: the byte board and one chunk more, so that the stream-out's fifth dword stays inside
__host__ __device__ inline uint32_t tp_wave_lds(const int NN) { return tp_board_bytes(NN) + 16u; }

// bytes of one tree of S_cap + 1 nodes (host and device agree on it here and nowhere else)
__host__ __device__ inline uint64_t tp_tree_bytes(const int S_cap, const int NN)
{
    const uint64_t N = (uint64_t)S_cap + 1u;
    return ((uint64_t)TP_FIXED_BYTES + tp_board_bytes(NN) + N * 22u + 15u) & ~(uint64_t)15u;
}

struct tp_tree {
    uint32_t *hdr, *players;
    uint8_t *board;
    uint32_t *n, *w;
    uint16_t *prior, *child, *path;
};

__device__ __forceinline__ tp_tree tp_tree_of(uint8_t *trees, const int64_t b, const uint64_t tree_bytes, const int S_cap, const int NN)
{
    uint8_t *base = trees + (uint64_t)b * tree_bytes;
    const uint32_t N = (uint32_t)S_cap + 1u;
    tp_tree t;
    t.hdr = reinterpret_cast<uint32_t *>(base);
    t.players = reinterpret_cast<uint32_t *>(base + TP_HDR_BYTES);
    t.board = base + TP_FIXED_BYTES;
    t.n = reinterpret_cast<uint32_t *>(base + TP_FIXED_BYTES + tp_board_bytes(NN));
    t.w = t.n + N;
    t.prior = reinterpret_cast<uint16_t *>(t.w + N);
    t.child = t.prior + 3u * N;
    t.path = t.child + 3u * N;
    return t;
}

__device__ __forceinline__ void tp_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// floor(num / den) for num < 2^52 and 1 <= den < 2^32 (the double quotient is within one of it, the remainder decides) and
// the exact floor square root of x < 2^52: tm_div / tm_isqrt of tron_mcts.hip
__device__ __forceinline__ uint64_t tp_div(const uint64_t num, const uint32_t den)
{
    uint64_t q = (uint64_t)((double)num / (double)den);
    const int64_t r = (int64_t)(num - q * (uint64_t)den);
    q = r < 0 ? q - 1u : (r >= (int64_t)den ? q + 1u : q);
    return q;
}

__device__ __forceinline__ uint64_t tp_isqrt(const uint64_t x)
{
    uint64_t s = (uint64_t)sqrt((double)x);
    s = s * s > x ? s - 1u : ((s + 1u) * (s + 1u) <= x ? s + 1u : s);
    return s;
}

// a wave-uniform word in a vector register (ttt_in_vgpr of ttt.hip): the player vectors are alike in every lane, and left to
// the compiler they went to scalar registers, of which the eight-player descent then spilled 246
__device__ __forceinline__ uint32_t tp_in_vgpr(const uint32_t x)
{
    uint32_t v;
    asm("v_mov_b32 %0, %1" : "=v"(v) : "s"(x));
    return v;
}

template <typename T>
__device__ __forceinline__ T *tp_ptr_in_vgpr(T *p)
{
    const uint64_t a = reinterpret_cast<uint64_t>(p);
    return reinterpret_cast<T *>(((uint64_t)tp_in_vgpr((uint32_t)(a >> 32)) << 32) | (uint64_t)tp_in_vgpr((uint32_t)a));
}

// 1 where a == b, else 0, without a compare
__device__ __forceinline__ uint32_t tp_eq01(const uint32_t a, const uint32_t b)
{
    const uint32_t x = a ^ b;
    return ((x | (0u - x)) >> 31) ^ 1u;
}

// a position without its board: heads (flat and split), directions, deaths (0 alive, else the 1-based killer id)
template <int P>
struct TpPos {
    int h[P], x[P], y[P], d[P], k[P];
};

template <int P>
__device__ __forceinline__ uint32_t tp_alive(const TpPos<P> &s)
{
    uint32_t alive = 0u;
#pragma unroll
    for (int p = 0; p < P; ++p) alive |= (s.k[p] == 0 ? 1u : 0u) << p;
    return alive;
}

// the cell next to (hx, hy) in direction dir, clamped onto the board (TronGridEnvironment.py:467-481)
__device__ __forceinline__ int tp_avoid_cell(const int N, const int hx, const int hy, const int dir)
{
    const int dd = dir & 3;
    const int nx = min(max(hx + (dd == 1) - (dd == 3), 0), N - 1);
    const int ny = min(max(hy + (dd == 2) - (dd == 0), 0), N - 1);
    return ny * N + nx;
}

// crl_tron_sample_avoid's rule for every live player on the pre-step byte board, under the avoid playout tag with the tree
// steps' third counter word: code 0 forward, 1 right, 3 left (the step's encoding); dead players get 0
template <int P>
__device__ __forceinline__ void tp_avoid_codes(const int N, const int NN, const int8_t *bd, const TpPos<P> &s, const uint32_t gid,
                                               const uint32_t c, const uint32_t k0, const uint32_t k1, const uint64_t thr, int (&code)[P])
{
#pragma unroll
    for (int p = 0; p < P; ++p) {                               // (a dead player's probes and draw are made and dropped: no branch)
        const int c_f = tp_avoid_cell(N, s.x[p], s.y[p], s.d[p]);
        const int c_r = tp_avoid_cell(N, s.x[p], s.y[p], s.d[p] + 1);
        const int c_l = tp_avoid_cell(N, s.x[p], s.y[p], s.d[p] + 3);
        CRL_BOUNDS_LT(c_f, NN, 192);
        CRL_BOUNDS_LT(c_r, NN, 192);
        CRL_BOUNDS_LT(c_l, NN, 192);
        (void)NN;
        const int o_f = bd[c_f] > 0, o_r = bd[c_r] > 0, o_l = bd[c_l] > 0;
        const philox_out wv = philox4x32_10(gid, c, TP_TREE_STEP, CRL_TAG_TRON_AVOID_PLAYOUT | (uint32_t)p, k0, k1);
        const uint32_t a3 = __umulhi(wv.w[1], 3u);
        const bool left_first = (wv.w[2] >> 31) != 0u;
        const bool first_free = (left_first ? o_l : o_r) == 0;
        const int side = (left_first == first_free) ? 3 : 1;
        const int a = ((uint64_t)wv.w[0] < thr) ? (int)(a3 + (a3 >> 1)) : (o_f == 0 ? 0 : side);
        code[p] = s.k[p] == 0 ? a : 0;
        // one player's block at a time (eight scheduled side by side: 203 against 195 vector registers in the 8-player instance)
        __builtin_amdgcn_sched_barrier(0);
    }
}

// the random agent at step counter c: crl_tron_rollout's digit rule with j = c & 7 under the random playout tag (players
// 0..3 and, with P > 4, players 4..7 from a second block); a code for every player (the dead ones' are not used)
template <int P>
__device__ __forceinline__ void tp_random_codes(const uint32_t gid, const uint32_t c, const uint32_t k0, const uint32_t k1, int (&code)[P])
{
    const uint32_t sel = (c & 7u) >> 1;
    const philox_out wa = philox4x32_10(gid, c >> 3, TP_TREE_STEP, CRL_TAG_TRON_PLAYOUT, k0, k1);
    const uint32_t word_a = sel == 0u ? wa.w[0] : sel == 1u ? wa.w[1] : sel == 2u ? wa.w[2] : wa.w[3];
    uint32_t word_b = 0u;
    if constexpr (P > 4) {
        const philox_out wb = philox4x32_10(gid, c >> 3, TP_TREE_STEP, CRL_TAG_TRON_PLAYOUT | 1u, k0, k1);
        word_b = sel == 0u ? wb.w[0] : sel == 1u ? wb.w[1] : sel == 2u ? wb.w[2] : wb.w[3];
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const uint32_t lo3 = (p & 3) == 0 ? 1u : (p & 3) == 1 ? 3u : (p & 3) == 2 ? 9u : 27u;    // 3^(p & 3), 3^(4 + (p & 3))
        const uint32_t v = (p < 4 ? word_a : word_b) * ((c & 1u) ? 81u * lo3 : lo3);
        const uint32_t a3 = __umulhi(v, 3u);
        code[p] = (int)(a3 + (a3 >> 1));
    }
}

// crl_tron_step without reset on the byte board WITH OWNERS, in the reference's sequential order (CyTronGrid.pyx:15-62):
// tm_step's straight-line selects (tron_mcts.hip), one LDS byte read and write per player (rewriting an unchanged byte is
// harmless: the board is the wave's own).  A crash takes the cell's value as the killer id; the owner dies too when its head
// is on that cell, and gets the mover's id, whether it was alive or not (as :56-57 writes it).
template <int P>
__device__ __forceinline__ void tp_step(const int N, const int NN, int8_t *bd, TpPos<P> &s, const int (&code)[P])
{
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const bool run = s.k[i] == 0;                            // (may have been killed head-on by j < i)
        const int dir = (s.d[i] + code[i]) & 3;
        s.d[i] = run ? dir : s.d[i];
        const int nx = s.x[i] + (dir == 1) - (dir == 3);
        const int ny = s.y[i] + (dir == 2) - (dir == 0);
        const bool oob = (unsigned)nx >= (unsigned)N || (unsigned)ny >= (unsigned)N;
        const int cell = oob ? s.h[i] : ny * N + nx;
        CRL_BOUNDS_LT(cell, NN, 193);
        (void)NN;
        const int val = bd[cell];
        const bool occupied = val > 0;
        const bool crash = run & !oob & occupied;
        const bool moved = run & !oob & !occupied;
        s.k[i] = run ? (oob ? i + 1 : (occupied ? val : 0)) : s.k[i];
        // head-on: the owner dies too when its head is on the cell, whether it was alive or not (as :56-57 writes it), in
        // 0 / 1 words
        const uint32_t crashed = crash ? 1u : 0u;
#pragma unroll
        for (int o = 0; o < P; ++o) {
            const uint32_t hit = crashed & tp_eq01((uint32_t)val, (uint32_t)(o + 1)) & tp_eq01((uint32_t)s.h[o], (uint32_t)cell);
            s.k[o] += (int)hit * (i + 1 - s.k[o]);
        }
        bd[cell] = (int8_t)(moved ? i + 1 : val);
        s.h[i] = moved ? cell : s.h[i];
        s.x[i] = moved ? nx : s.x[i];
        s.y[i] = moved ? ny : s.y[i];
        // the deaths are settled here, in their registers: left alone the compiler carries every earlier mover's crash mask
        // (two scalar registers each) to the turn of the player it might have killed, and the eight-player descent spills
#pragma unroll
        for (int o = 0; o < P; ++o) asm volatile("" : "+v"(s.k[o]));
        asm volatile("" : "+v"(s.h[i]), "+v"(s.x[i]), "+v"(s.y[i]), "+v"(s.d[i]));     // (and the mover's own vectors, for its move mask)
    }
}

// the relative-player transform of one dword of cells (crl_tron_observe's board rule: v > 0 -> ((v - (seat + 1) + P) % P) + 1,
// other values as they are); the seat of a live tree is in [0, P), so the dividend is positive
template <int P>
__device__ __forceinline__ uint32_t tp_relative4(const uint32_t cells, const int seat)
{
    uint32_t out = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int v = (int)(int8_t)(cells >> (8 * i));
        const int r = v > 0 ? (int)((uint32_t)(v - (seat + 1) + P) % (uint32_t)P) + 1 : v;
        out |= ((uint32_t)r & 255u) << (8 * i);
    }
    return out;
}

// One row of NN cells out of the wave's LDS board `bd` (16-byte aligned, tp_wave_lds bytes) to dst, which starts anywhere:
// single bytes up to the first 16-byte boundary (lanes 0..15) and behind the last whole chunk (lanes 16..31), aligned
// 16-byte stores between, lanes over chunks.  A chunk's 16 bytes start at any LDS byte: five aligned dwords and a byte
// funnel.  RELATIVE: through the relative-player transform.  zero: the row is zeros.  Nothing is stored outside the row.
template <int P, bool RELATIVE>
__device__ __forceinline__ void tp_stream_row(int8_t *dst, const int NN, const uint8_t *bd, int lane, const int seat, const bool zero)
{
    asm volatile("" : "+v"(lane));                              // (its compares are made here, not kept in scalar pairs from the kernel's start)
    const int mis = (int)(reinterpret_cast<uintptr_t>(dst) & 15u);
    const int head = min(NN, (16 - mis) & 15);
    const int nch = (NN - head) >> 4, tail0 = head + (nch << 4);
    const int edge = lane < 16 ? lane : tail0 + (lane - 16);
    if (lane < 16 ? lane < head : (lane < 32 && edge < NN)) {
        CRL_BOUNDS_LT(edge, NN, 194);
        const uint32_t v = zero ? 0u : (uint32_t)bd[edge];
        dst[edge] = (int8_t)(RELATIVE ? tp_relative4<P>(v, seat) : v);
    }
    for (int j = lane; j < nch; j += 64) {
        const int o = head + (j << 4), a = o & ~3, sh = 8 * (o & 3);
        CRL_BOUNDS_LT(a + 19, (int)tp_wave_lds(NN), 195);
        uint4 q = make_uint4(0u, 0u, 0u, 0u);
        if (!zero) {
            const uint32_t *src = reinterpret_cast<const uint32_t *>(bd + a);
            const uint32_t d0 = src[0], d1 = src[1], d2 = src[2], d3 = src[3], d4 = src[4];
            q.x = (uint32_t)((((uint64_t)d1 << 32) | d0) >> sh);
            q.y = (uint32_t)((((uint64_t)d2 << 32) | d1) >> sh);
            q.z = (uint32_t)((((uint64_t)d3 << 32) | d2) >> sh);
            q.w = (uint32_t)((((uint64_t)d4 << 32) | d3) >> sh);
            if (RELATIVE) {
                q.x = tp_relative4<P>(q.x, seat); q.y = tp_relative4<P>(q.y, seat);
                q.z = tp_relative4<P>(q.z, seat); q.w = tp_relative4<P>(q.w, seat);
            }
        }
        *reinterpret_cast<uint4 *>(dst + o) = q;
    }
}

// ---- begin: the header, the root position and the root node of every tree
template <int P>
__global__ void __launch_bounds__(256)
tron_puct_begin_kernel(const int N, const int NN, const int64_t B, const uint32_t seed_lo, const uint32_t seed_hi,
                       const uint64_t first_env_id, const int8_t *__restrict__ board, const int16_t *__restrict__ heads,
                       const int8_t *__restrict__ dirs, const int8_t *__restrict__ deaths, const uint32_t *__restrict__ tcount,
                       const int8_t *__restrict__ seat_in, const uint32_t model, const uint64_t thr, uint8_t *__restrict__ trees,
                       const uint64_t tree_bytes, const int S_cap)
{
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    for (int64_t b = (int64_t)blockIdx.x * 4 + wave; b < B; b += (int64_t)gridDim.x * 4) {
        const tp_tree t = tp_tree_of(trees, b, tree_bytes, S_cap, NN);
        const int sp = seat_in ? (int)seat_in[b] : 0;
        uint32_t alive = 0u;
#pragma unroll
        for (int p = 0; p < P; ++p) alive |= (deaths[p * B + b] == 0 ? 1u : 0u) << p;
        // crl_tron_mcts's skip rule
        const bool live = (unsigned)sp < (unsigned)P && ((alive >> (sp & 7)) & 1u) && (P == 1 || __popc(alive) >= 2);
        uint32_t word = 0u;
        if (lane == TP_H_NODES) word = live ? 1u : 0u;
        if (lane == TP_H_SEAT) word = live ? (uint32_t)sp : 0u;
        if (lane == TP_H_TCOUNT) word = tcount ? tcount[b] : 0u;
        if (lane == TP_H_GID) word = (uint32_t)(first_env_id + (uint64_t)b);
        if (lane == TP_H_SEED_LO) word = seed_lo;
        if (lane == TP_H_SEED_HI) word = seed_hi;
        if (lane == TP_H_MODEL) word = model;
        if (lane == TP_H_THR_LO) word = (uint32_t)thr;
        if (lane == TP_H_THR_HI) word = (uint32_t)(thr >> 32);
        if (lane < TP_HDR_BYTES / 4) t.hdr[lane] = word;
        if (lane < CRL_TRON_MAX_P) {
            uint32_t pw = 0u;
            if (lane < P) {
                const int64_t at = (int64_t)lane * B + b;
                const uint32_t h = (uint32_t)min(max((int)heads[at], 0), NN - 1);     // crl_tron_playout's precondition
                pw = h | ((uint32_t)(dirs[at] & 3) << 16) | (((uint32_t)deaths[at] & 255u) << 24);
            }
            t.players[lane] = pw;
        }
        const int NNp = (int)tp_board_bytes(NN);
        // lanes over 16-byte chunks: the game's row starts anywhere, so a chunk is gathered byte by byte (bytes past the row: 0),
        // the tree's copy is 16-byte aligned and stored whole
        for (int j = lane; j < (NNp >> 4); j += 64) {
            uint32_t q[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int c = (j << 4) + i;
                const uint32_t v = c < NN ? (uint32_t)(uint8_t)board[b * NN + c] : 0u;
                q[i >> 2] |= v << (8 * (i & 3));
            }
            reinterpret_cast<uint4 *>(t.board)[j] = make_uint4(q[0], q[1], q[2], q[3]);
        }
        if (lane == 0) { t.n[0] = 0u; t.w[0] = 0u; t.path[0] = 0; }
        if (lane < 3) { t.prior[lane] = 0; t.child[lane] = 0; }
    }
}

// ---- select: one descent of every tree on a byte board in LDS, the leaf out in observation layout
template <int P>
__global__ void __launch_bounds__(256)
tron_puct_select_kernel(const int N, const int NN, const uint32_t inv_n, const int64_t B, uint8_t *trees_arg,
                        const uint64_t tree_bytes, const int S_cap, const uint32_t cpuct, const uint32_t fpu,
                        int8_t *obs_board_arg, int16_t *obs_heads_arg, int8_t *obs_dirs_arg, int8_t *obs_deaths_arg,
                        uint8_t *pending_arg, uint32_t *depth_arg, int8_t *leaf_board_arg, int16_t *leaf_heads_arg,
                        int8_t *leaf_dirs_arg, int8_t *leaf_deaths_arg)
{
    // the ten output pointers wait for the end of a descent in vector registers: left where the arguments arrive, they and
    // the descent's scalars did not fit and the eight-player instance spilled 94 scalar registers
    int8_t *const obs_board = tp_ptr_in_vgpr(obs_board_arg), *const obs_dirs = tp_ptr_in_vgpr(obs_dirs_arg),
                 *const obs_deaths = tp_ptr_in_vgpr(obs_deaths_arg), *const leaf_board = tp_ptr_in_vgpr(leaf_board_arg),
                 *const leaf_dirs = tp_ptr_in_vgpr(leaf_dirs_arg), *const leaf_deaths = tp_ptr_in_vgpr(leaf_deaths_arg);
    int16_t *const obs_heads = tp_ptr_in_vgpr(obs_heads_arg), *const leaf_heads = tp_ptr_in_vgpr(leaf_heads_arg);
    uint8_t *const pending_g = tp_ptr_in_vgpr(pending_arg);
    uint32_t *const depth_g = tp_ptr_in_vgpr(depth_arg);
    uint8_t *const trees = tp_ptr_in_vgpr(trees_arg);           // (and so do the tree's seven array pointers)
    extern __shared__ __attribute__((aligned(16))) uint8_t tp_lds[];
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), n_waves = (int)(blockDim.x >> 6);
    uint8_t *const bd_u = tp_lds + (uint32_t)wave * tp_wave_lds(NN);
    int8_t *const bd = reinterpret_cast<int8_t *>(bd_u);
    const int nchunks = (int)(tp_board_bytes(NN) >> 4);

    for (int64_t b = (int64_t)blockIdx.x * n_waves + wave; b < B; b += (int64_t)gridDim.x * n_waves) {
        const tp_tree t = tp_tree_of(trees, b, tree_bytes, S_cap, NN);
        uint32_t nn = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.hdr[TP_H_NODES]);
        const uint32_t sims = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.hdr[TP_H_SIMS]);
        const int sp = min(__builtin_amdgcn_readfirstlane((int)(t.hdr[TP_H_SEAT] & 7u)), P - 1);
        TpPos<P> ps;
#pragma unroll
        for (int p = 0; p < P; ++p) { ps.h[p] = 0; ps.x[p] = 0; ps.y[p] = 0; ps.d[p] = 0; ps.k[p] = 0; }
        bool pend = false;
        int d = 0;
        tp_wave_sync();                                          // the last tree's stream-out has read the board
        if (nn != 0u && nn <= (uint32_t)S_cap + 1u && sims < (uint32_t)S_cap) {     // (a skipped or a full tree is left alone)
            // ---- the root position: the board in aligned 16-byte chunks, lanes over chunks; the players alike in every lane
            for (int j = lane; j < nchunks; j += 64)
                reinterpret_cast<uint4 *>(bd_u)[j] = reinterpret_cast<const uint4 *>(t.board)[j];
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const uint32_t pw = tp_in_vgpr((uint32_t)__builtin_amdgcn_readfirstlane((int)t.players[p]));
                ps.h[p] = min((int)(pw & 0xffffu), NN - 1);
                ps.y[p] = (int)__umulhi((uint32_t)ps.h[p], inv_n);
                ps.x[p] = ps.h[p] - ps.y[p] * N;
                ps.d[p] = (int)((pw >> 16) & 3u);
                ps.k[p] = (int)(int8_t)(pw >> 24);
            }
            // (the draws' inputs too: eight Philox blocks side by side in scalar registers do not fit either)
            const uint32_t tc = tp_in_vgpr((uint32_t)__builtin_amdgcn_readfirstlane((int)t.hdr[TP_H_TCOUNT]));
            const uint32_t gid = tp_in_vgpr((uint32_t)__builtin_amdgcn_readfirstlane((int)t.hdr[TP_H_GID]));
            const uint32_t k0 = tp_in_vgpr((uint32_t)__builtin_amdgcn_readfirstlane((int)t.hdr[TP_H_SEED_LO]));
            const uint32_t k1 = tp_in_vgpr((uint32_t)__builtin_amdgcn_readfirstlane((int)t.hdr[TP_H_SEED_HI]));
            const bool avoid = __builtin_amdgcn_readfirstlane((int)t.hdr[TP_H_MODEL]) != 0;
            const uint64_t thr = ((uint64_t)t.hdr[TP_H_THR_HI] << 32) | (uint64_t)t.hdr[TP_H_THR_LO];
            uint32_t is_seat[P];
#pragma unroll
            for (int p = 0; p < P; ++p) is_seat[p] = tp_in_vgpr(p == sp ? 1u : 0u);
            tp_wave_sync();
            int v = 0, term = 0, seat_alive = 1;
            for (;;) {
                CRL_BOUNDS_LT(v, S_cap + 1, 196);
                const uint32_t nv = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.n[v]);
                if (nv == 0u) { pend = true; break; }           // an unexpanded node: the pending leaf
                if (d >= S_cap) break;                           // (never: a path of d edges has d + 1 distinct nodes)
                // ---- lane a scores the child at action a
                const size_t at = (size_t)v * 3u + (size_t)(lane < 3 ? lane : 0);
                const uint32_t pe = lane < 3 ? t.prior[at] : 0u;
                uint32_t cu = lane < 3 ? t.child[at] : 0u;
                CRL_BOUNDS_LT(cu, S_cap + 1, 197);
                cu = min(cu, (uint32_t)S_cap);
                const uint64_t rt = tp_isqrt((uint64_t)min(nv, 4095u) << 16);
                uint32_t key = 0u;
                if (lane < 3) {
                    const uint32_t nu = cu ? min(t.n[cu], 4095u) : 0u, wu = cu ? t.w[cu] : 0u;   // (n <= S_cap: den < 2^32)
                    const uint64_t exploit = nu ? tp_div(wu, nu) : (uint64_t)fpu;
                    const uint64_t explore = tp_div((uint64_t)cpuct * pe * rt, (1u + nu) << 16);
                    key = (uint32_t)min(exploit + explore, (uint64_t)0x7fffffffu);               // score < 2^16 + 2^30
                }
                // the arg-max over the three lanes, ties to the lowest action (every lane runs the reads)
                const uint32_t key0 = (uint32_t)__builtin_amdgcn_readlane((int)key, 0), key1 = (uint32_t)__builtin_amdgcn_readlane((int)key, 1),
                               key2 = (uint32_t)__builtin_amdgcn_readlane((int)key, 2);
                const int e = key1 > key0 ? (key2 > key1 ? 2 : 1) : (key2 > key0 ? 2 : 0);
                const int c0 = __builtin_amdgcn_readlane((int)cu, 0), c1 = __builtin_amdgcn_readlane((int)cu, 1),
                          c2 = __builtin_amdgcn_readlane((int)cu, 2);
                int u = e == 0 ? c0 : e == 1 ? c1 : c2;
                const bool fresh = u == 0;
                if (fresh) {
                    if (nn > (uint32_t)S_cap) break;             // (never: nodes <= simulations + 1 <= S_cap)
                    u = (int)nn++;
                    CRL_BOUNDS_LT(u, S_cap + 1, 198);
                    if (lane == e) t.child[at] = (uint16_t)u;
                    if (lane < 3) { t.prior[(size_t)u * 3u + lane] = 0; t.child[(size_t)u * 3u + lane] = 0; }
                    if (lane == 0) { t.n[u] = 0u; t.w[u] = 0u; }
                }
                // ---- the tree step at depth d: the seat plays e, the others the model agent on the pre-step position
                int code[P];
                const uint32_t c = tc + (uint32_t)d;
                if (avoid) {
                    tp_avoid_codes<P>(N, NN, bd, ps, gid, c, k0, k1, thr, code);
                } else {
                    tp_random_codes<P>(gid, c, k0, k1, code);
                }
                // (the seat's code by arithmetic on a 0 / 1 word per player: a compare with the seat is loop-invariant, and its
                // lane mask would wait in two scalar registers per player)
#pragma unroll
                for (int p = 0; p < P; ++p) code[p] += (int)is_seat[p] * (e + (e >> 1) - code[p]);
                tp_step<P>(N, NN, bd, ps, code);
                d += 1;
                CRL_BOUNDS_LT(d, S_cap + 1, 199);
                if (lane == 0) t.path[d] = (uint16_t)u;
                const uint32_t alive = tp_alive<P>(ps);
                seat_alive = __builtin_amdgcn_readfirstlane((int)((alive >> sp) & 1u));
                term = (!seat_alive || __builtin_amdgcn_readfirstlane(__popc(alive)) <= 1) ? 1 : 0;   // CLOSED, crl_tron_mcts's rule
                if (term) break;
                if (fresh) { pend = true; break; }               // the new node is the leaf: nothing of it is read back
                v = u;
            }
            const bool have = pend || term;
            if (lane == 0) {
                t.path[0] = 0;
                t.hdr[TP_H_NODES] = nn;
                t.hdr[TP_H_PATH] = have ? (uint32_t)d + 1u : 0u;
                t.hdr[TP_H_LEAF] = (pend ? TP_PENDING : TP_TERMINAL) | ((uint32_t)seat_alive << 8);
            }
        } else if (nn != 0u && nn <= (uint32_t)S_cap + 1u) {
            if (lane == 0) t.hdr[TP_H_PATH] = 0u;                // at capacity: no path
        }
        // ---- the outputs: the pending leaf as the seat sees it (crl_tron_observe with player = seat), zeros for the rest
        tp_wave_sync();
        tp_stream_row<P, true>(obs_board + b * NN, NN, bd_u, lane, sp, !pend);
        if (leaf_board != nullptr) tp_stream_row<P, false>(leaf_board + b * NN, NN, bd_u, lane, sp, !pend);
        // (lane 0 writes the player rows one by one: the vectors are alike in every lane, and a lane-per-player gather keeps
        // two lane masks per player in scalar registers across the whole kernel)
        int sp_out = sp;
        asm volatile("" : "+v"(sp_out));                         // (its compares are made here, behind the descent)
        sp_out = __builtin_amdgcn_readfirstlane(sp_out);
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < P; ++i) {
                int src = i + sp_out;
                src = src >= P ? src - P : src;
                int oh = 0, od = 0, ok = 0;
#pragma unroll
                for (int p = 0; p < P; ++p) { oh = p == src ? ps.h[p] : oh; od = p == src ? ps.d[p] : od; ok = p == src ? ps.k[p] : ok; }
                const int64_t at = (int64_t)i * B + b;
                obs_heads[at] = (int16_t)(pend ? oh : 0);
                obs_dirs[at] = (int8_t)(pend ? od : 0);
                obs_deaths[at] = (int8_t)(pend ? ok : 0);
                if (leaf_board != nullptr) {
                    leaf_heads[at] = (int16_t)(pend ? ps.h[i] : 0);
                    leaf_dirs[at] = (int8_t)(pend ? ps.d[i] : 0);
                    leaf_deaths[at] = (int8_t)(pend ? ps.k[i] : 0);
                }
            }
        }
        if (lane == 0) {
            pending_g[b] = pend ? 1 : 0;
            depth_g[b] = pend ? (uint32_t)d : 0u;
        }
    }
}

// ---- backup: the leaf's priors, then lane i adds to the node at depth i of the path (distinct nodes: no atomics), 64 per pass
__global__ void __launch_bounds__(256)
tron_puct_backup_kernel(const int NN, const int64_t B, uint8_t *__restrict__ trees, const uint64_t tree_bytes, const int S_cap,
                        const uint16_t *__restrict__ prior_g, const int32_t *__restrict__ value_g)
{
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    for (int64_t b = (int64_t)blockIdx.x * 4 + wave; b < B; b += (int64_t)gridDim.x * 4) {
        const tp_tree t = tp_tree_of(trees, b, tree_bytes, S_cap, NN);
        const uint32_t nn = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.hdr[TP_H_NODES]);
        const int plen = __builtin_amdgcn_readfirstlane((int)t.hdr[TP_H_PATH]);
        if (nn == 0u || plen <= 0 || plen > S_cap + 1) continue;                    // skipped, or no path outstanding: left alone
        const uint32_t sims = t.hdr[TP_H_SIMS], leaf = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.hdr[TP_H_LEAF]);
        const bool pend = (leaf & 3u) == TP_PENDING;
        uint32_t add = ((leaf >> 8) & 1u) ? 65536u : 0u;         // a terminal leaf: the seat alive or not
        if (pend) {
            CRL_BOUNDS_LT(t.path[plen - 1], S_cap + 1, 165);
            const uint32_t L = min((uint32_t)t.path[plen - 1], (uint32_t)S_cap);
            const uint32_t pr = lane < 3 ? prior_g[b * 3 + lane] : 0u;
            const uint32_t sum = (uint32_t)__builtin_amdgcn_readlane((int)pr, 0) + (uint32_t)__builtin_amdgcn_readlane((int)pr, 1) +
                                 (uint32_t)__builtin_amdgcn_readlane((int)pr, 2);
            const uint32_t slot = (uint32_t)min((uint64_t)65535u, sum ? tp_div((uint64_t)pr << 16, max(sum, 1u)) : (uint64_t)(65536u / 3u));
            if (lane < 3) t.prior[(size_t)L * 3u + lane] = (uint16_t)slot;
            add = (uint32_t)min(max(value_g[b], 0), 65536);
        }
        for (int i0 = 0; i0 < plen; i0 += 64) {
            const int i = i0 + lane;
            if (i < plen) {
                CRL_BOUNDS_LT(t.path[i], S_cap + 1, 166);
                const uint32_t node = min((uint32_t)t.path[i], (uint32_t)S_cap);
                t.n[node] += 1u;
                if (i > 0) t.w[node] += add;
            }
        }
        if (lane == 0) { t.hdr[TP_H_SIMS] = sims + 1u; t.hdr[TP_H_PATH] = 0u; }
    }
}

// ---- root: the root's children, its priors, the counts and the most visited action (then the larger w, then the lower action)
__global__ void __launch_bounds__(256)
tron_puct_root_kernel(const int NN, const int64_t B, uint8_t *__restrict__ trees, const uint64_t tree_bytes, const int S_cap,
                      uint32_t *__restrict__ visits, uint32_t *__restrict__ value, uint32_t *__restrict__ prior_out,
                      uint32_t *__restrict__ nodes, uint32_t *__restrict__ sims_out, int32_t *__restrict__ best)
{
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    for (int64_t b = (int64_t)blockIdx.x * 4 + wave; b < B; b += (int64_t)gridDim.x * 4) {
        const tp_tree t = tp_tree_of(trees, b, tree_bytes, S_cap, NN);
        const uint32_t nn = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.hdr[TP_H_NODES]);
        const bool live = nn != 0u;
        uint32_t cu = live && lane < 3 ? t.child[lane] : 0u;
        CRL_BOUNDS_LT(cu, S_cap + 1, 167);
        cu = min(cu, (uint32_t)S_cap);
        const uint32_t vis = cu ? t.n[cu] : 0u, val = cu ? t.w[cu] : 0u;
        if (lane < 3) {
            visits[b * 3 + lane] = vis;
            value[b * 3 + lane] = val;
            prior_out[b * 3 + lane] = live ? t.prior[lane] : 0u;
        }
        int pick = -1;
        uint32_t pick_n = 0u, pick_w = 0u;
#pragma unroll
        for (int a = 0; a < 3; ++a) {                            // (every lane runs the reads)
            const uint32_t na = (uint32_t)__builtin_amdgcn_readlane((int)vis, a), wa = (uint32_t)__builtin_amdgcn_readlane((int)val, a);
            const bool better = na != 0u && (pick < 0 || na > pick_n || (na == pick_n && wa > pick_w));
            pick = better ? a : pick;
            pick_n = better ? na : pick_n;
            pick_w = better ? wa : pick_w;
        }
        if (lane == 0) {
            nodes[b] = nn;
            sims_out[b] = live ? t.hdr[TP_H_SIMS] : 0u;
            best[b] = pick;
        }
    }
}

inline unsigned tp_blocks(const int64_t B, const uint32_t waves)
{
    const uint64_t want = ((uint64_t)B + waves - 1u) / waves;
    return (unsigned)(want < (1u << 20) ? want : (1u << 20));    // (a grid-stride loop past that)
}

} // namespace

// the checks every entry shares: the context, B, the tree pointer, S_cap, the board against LDS
#define TP_CHECK(fn)                                                                                                   \
    TRON_CTX_CHECK(fn);                                                                                                \
    CRL_REQUIRE(tree != nullptr, fn ": NULL tree pointer");                                                            \
    CRL_REQUIRE((((uintptr_t)tree) & 15) == 0, fn ": tree must be 16-byte aligned");                                   \
    CRL_REQUIRE(S_cap >= 1 && S_cap <= TP_MAX_S, fn ": S_cap=%d out of range 1..%d", S_cap, TP_MAX_S);                 \
    const crl_tron_cfg &cfg = ctx->tron;                                                                               \
    const int NN = cfg.N * cfg.N;                                                                                      \
    if (tp_wave_lds(NN) > TP_LDS) {                                                                                    \
        crl_set_error(fn ": the byte copy of a %dx%d board does not fit one workgroup's LDS", cfg.N, cfg.N);           \
        return CRL_EUNSUPPORTED;                                                                                       \
    }                                                                                                                  \
    const uint64_t tree_bytes = tp_tree_bytes(S_cap, NN);                                                              \
    uint8_t *trees = static_cast<uint8_t *>(tree);                                                                     \
    hipStream_t st = (hipStream_t)stream

int crl_tron_puct_bounds(unsigned int *out4)
{
    CRL_BOUNDS_READBACK(out4);
    return CRL_OK;
}

extern "C" {

int64_t crl_tron_puct_tree_bytes(const crl_ctx *ctx, int S_cap)
{
    CRL_REQUIRE(ctx != nullptr && ctx->game == CRL_GAME_TRON, "crl_tron_puct_tree_bytes: ctx is not a tron context");
    CRL_REQUIRE(S_cap >= 1 && S_cap <= TP_MAX_S, "crl_tron_puct_tree_bytes: S_cap=%d out of range 1..%d", S_cap, TP_MAX_S);
    return (int64_t)tp_tree_bytes(S_cap, ctx->tron.N * ctx->tron.N);
}

int crl_tron_puct_begin(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, const int8_t *board, const int16_t *heads,
                        const int8_t *dirs, const int8_t *deaths, const uint32_t *tcount, const int8_t *seat, int S_cap, double noise,
                        uint32_t flags, void *tree, void *stream)
{
    TP_CHECK("crl_tron_puct_begin");
    CRL_REQUIRE(board && heads && dirs && deaths, "crl_tron_puct_begin: NULL state pointer");
    CRL_REQUIRE(noise >= 0.0 && noise <= 1.0, "crl_tron_puct_begin: noise=%g not in [0, 1]", noise);
    CRL_REQUIRE((flags & ~CRL_PLAYOUT_AVOID) == 0u, "crl_tron_puct_begin: unknown flags 0x%x", flags);
    const uint64_t thr = crl_noise_threshold(noise);
    const uint32_t model = (flags & CRL_PLAYOUT_AVOID) ? 1u : 0u;
    TRON_DISPATCH_P(cfg.P, hipLaunchKernelGGL((tron_puct_begin_kernel<PP>), dim3(tp_blocks(B, 4u)), dim3(256), 0, st, cfg.N, NN, B,
                                              (uint32_t)seed, (uint32_t)(seed >> 32), first_env_id, board, heads, dirs, deaths, tcount,
                                              seat, model, thr, trees, tree_bytes, S_cap));
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

int crl_tron_puct_select(const crl_ctx *ctx, int64_t B, void *tree, int S_cap, uint32_t cpuct, uint32_t fpu, int8_t *obs_board,
                         int16_t *obs_heads, int8_t *obs_dirs, int8_t *obs_deaths, uint8_t *pending, uint32_t *depth,
                         int8_t *leaf_board, int16_t *leaf_heads, int8_t *leaf_dirs, int8_t *leaf_deaths, uint32_t flags, void *stream)
{
    TP_CHECK("crl_tron_puct_select");
    CRL_REQUIRE(obs_board && obs_heads && obs_dirs && obs_deaths && pending && depth, "crl_tron_puct_select: NULL output pointer");
    const int n_leaf = (leaf_board != nullptr) + (leaf_heads != nullptr) + (leaf_dirs != nullptr) + (leaf_deaths != nullptr);
    CRL_REQUIRE(n_leaf == 0 || n_leaf == 4, "crl_tron_puct_select: leaf_board / _heads / _dirs / _deaths must be all NULL or none");
    CRL_REQUIRE(cpuct <= 65535u, "crl_tron_puct_select: cpuct=%u out of range 0..65535", cpuct);
    CRL_REQUIRE(fpu <= 65536u, "crl_tron_puct_select: fpu=%u out of range 0..65536", fpu);
    CRL_REQUIRE(flags == 0, "crl_tron_puct_select: unknown flags 0x%x", flags);
    // one to four waves per workgroup, as many byte boards as fit in 64 KB, and no more than there are trees
    const uint32_t wave_bytes = tp_wave_lds(NN);
    uint32_t waves = TP_LDS / wave_bytes;
    waves = waves > 4u ? 4u : waves;
    waves = (int64_t)waves > B ? (uint32_t)B : waves;
    const uint32_t inv_n = (uint32_t)(0x100000000ull / (uint32_t)cfg.N) + 1u;   // y = umulhi(h, inv_n) is exact for h < N*N <= 2^15
    TRON_DISPATCH_P(cfg.P, hipLaunchKernelGGL((tron_puct_select_kernel<PP>), dim3(tp_blocks(B, waves)), dim3(64u * waves),
                                              (size_t)waves * wave_bytes, st, cfg.N, NN, inv_n, B, trees, tree_bytes, S_cap, cpuct, fpu,
                                              obs_board, obs_heads, obs_dirs, obs_deaths, pending, depth, leaf_board, leaf_heads,
                                              leaf_dirs, leaf_deaths));
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

int crl_tron_puct_backup(const crl_ctx *ctx, int64_t B, void *tree, int S_cap, const uint16_t *prior, const int32_t *value,
                         uint32_t flags, void *stream)
{
    TP_CHECK("crl_tron_puct_backup");
    CRL_REQUIRE(prior && value, "crl_tron_puct_backup: NULL input pointer");
    CRL_REQUIRE(flags == 0, "crl_tron_puct_backup: unknown flags 0x%x", flags);
    hipLaunchKernelGGL(tron_puct_backup_kernel, dim3(tp_blocks(B, 4u)), dim3(256), 0, st, NN, B, trees, tree_bytes, S_cap, prior, value);
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

int crl_tron_puct_root(const crl_ctx *ctx, int64_t B, void *tree, int S_cap, uint32_t *visits, uint32_t *value, uint32_t *prior,
                       uint32_t *nodes, uint32_t *sims, int32_t *best, void *stream)
{
    TP_CHECK("crl_tron_puct_root");
    CRL_REQUIRE(visits && value && prior && nodes && sims && best, "crl_tron_puct_root: NULL output pointer");
    hipLaunchKernelGGL(tron_puct_root_kernel, dim3(tp_blocks(B, 4u)), dim3(256), 0, st, NN, B, trees, tree_bytes, S_cap, visits, value,
                       prior, nodes, sims, best);
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

} // extern "C"
