// tron_puct_search.hip -- the whole network-valued Tron search in ONE launch (crl_tron_puct_search; the contract is in
// include/colosseum_hip.h), gfx950, wave64.  It leaves in the trees what n_sims repetitions of crl_tron_puct_select,
// crl_tron_net_eval and crl_tron_puct_backup leave, byte for byte: the descent and the backup are tron_puct.hip's statements,
// the MLP is tron_net.hip's arithmetic in tron_net.hip's order, restated here so that those kernels stay what they are.
// DESIGN.md 4.5p holds the layout, the LDS map and the measurements.
//
// A workgroup owns 16 trees -- one MFMA tile of leaves -- for all n_sims simulations, as 16 waves of one tree or as 8 waves of
// two (ts_waves_of: the 16-wave form caps a wave at 128 VGPRs, which no player count's descent fits without scratch).  A
// wave owns the same trees in every phase, so a tree's nodes are read and written by one wave only and HBM needs no ordering
// between waves.  A simulation is
//   1  descent (select's, wave-uniform, lanes 0..2 scoring) on the tree's WORKING BOARD in LDS, reset from a resident copy of
//      the root board by an LDS-to-LDS copy; the path goes to the tree as select writes it; the seat's head and facing and the
//      pending flag go to LDS tables                                                                   -> workgroup barrier
//   2  the MLP, dealt over the waves by OUTPUT tile (a run-time loop: no template over the width), the weights read from the
//      packed tile order through L2.  Every sum keeps crl_tron_net_eval's order: the bias first, then the k tiles ascending
//      (plane 0's cells, planes 1, 2, 3, the facing tile; inputs ascending in the later layers), four k-steps a tile.  No sum
//      is split over waves.  A barrier per layer; wave 0 computes the head tile and leaves three logits and the value of
//      every leaf in LDS.  Skipped when no leaf of the 16 is pending
//   3  epilogue and backup by the owning wave: exp / scale / round as tron_net_eval_kernel, backup's normalisation, the n / w
//      update along the path read back from the tree, 64 lanes a pass, the header words                 -> wave fence
// Leaves, priors and values never reach HBM.
//
// THE WORKING BOARD IS THE FIRST LAYER'S INPUT.  select hands the leaf out through the relative-player transform (the seat's
// trail becomes 1, anybody else's 2..P) and tn_plane_bits compares with constants; here the board keeps the absolute ids and
// the compares are made against the seat's id s = seat + 1:
//   empty  b == 0                (the observation: == 0)
//   own    b == s                (== 1)
//   other  1 <= b <= 127, b != s (> 1)
//   head   cell == the seat's head
// For every board with values in 0..P these are the same bits, so the products, their order and the results are the same.
// The bytes behind N N in a row are 255 (no feature), as in tron_net.hip.
// Unlike select and backup, the lanes of a wave here read through memory what other lanes wrote earlier in the launch (child
// slots, n / w, priors, the path): the wave fences order that.
#include "crl_common.hpp"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- the tree (tron_puct.hip states the layout)
constexpr int TS_H_NODES = 0, TS_H_SIMS = 1, TS_H_PATH = 2, TS_H_LEAF = 3, TS_H_SEAT = 4, TS_H_TCOUNT = 5, TS_H_GID = 6,
              TS_H_SEED_LO = 7, TS_H_SEED_HI = 8, TS_H_MODEL = 9, TS_H_THR_LO = 10, TS_H_THR_HI = 11;
constexpr int TS_HDR_BYTES = 64, TS_PLAYER_BYTES = 4 * CRL_TRON_MAX_P, TS_FIXED_BYTES = TS_HDR_BYTES + TS_PLAYER_BYTES;
constexpr uint32_t TS_PENDING = 1u, TS_TERMINAL = 2u;
constexpr int TS_MAX_S = 4095;
constexpr uint32_t TS_TREE_STEP = 0xFFFF0000u;                  // the third counter word of the tree steps' draws
static_assert(TS_FIXED_BYTES % 16 == 0 && CRL_TRON_MAX_P == 8, "a tree's fixed part");

__host__ __device__ inline uint32_t ts_pad16(const uint32_t x) { return (x + 15u) & ~15u; }

__host__ __device__ inline uint64_t ts_tree_bytes(const int S_cap, const int NN)
{
    const uint64_t N = (uint64_t)S_cap + 1u;
    return ((uint64_t)TS_FIXED_BYTES + ts_pad16((uint32_t)NN) + N * 22u + 15u) & ~(uint64_t)15u;
}

struct ts_tree {
    uint32_t *hdr, *players;
    uint8_t *board;
    uint32_t *n, *w;
    uint16_t *prior, *child, *path;
};

__device__ __forceinline__ ts_tree ts_tree_of(uint8_t *trees, const int64_t b, const uint64_t tree_bytes, const int S_cap, const int NN)
{
    uint8_t *base = trees + (uint64_t)b * tree_bytes;
    const uint32_t N = (uint32_t)S_cap + 1u;
    ts_tree t;
    t.hdr = reinterpret_cast<uint32_t *>(base);
    t.players = reinterpret_cast<uint32_t *>(base + TS_HDR_BYTES);
    t.board = base + TS_FIXED_BYTES;
    t.n = reinterpret_cast<uint32_t *>(base + TS_FIXED_BYTES + ts_pad16((uint32_t)NN));
    t.w = t.n + N;
    t.prior = reinterpret_cast<uint16_t *>(t.w + N);
    t.child = t.prior + 3u * N;
    t.path = t.child + 3u * N;
    return t;
}

__device__ __forceinline__ void ts_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// tp_div / tp_isqrt of tron_puct.hip
__device__ __forceinline__ uint64_t ts_div(const uint64_t num, const uint32_t den)
{
    uint64_t q = (uint64_t)((double)num / (double)den);
    const int64_t r = (int64_t)(num - q * (uint64_t)den);
    q = r < 0 ? q - 1u : (r >= (int64_t)den ? q + 1u : q);
    return q;
}

__device__ __forceinline__ uint64_t ts_isqrt(const uint64_t x)
{
    uint64_t s = (uint64_t)sqrt((double)x);
    s = s * s > x ? s - 1u : ((s + 1u) * (s + 1u) <= x ? s + 1u : s);
    return s;
}

// a wave-uniform word in a vector register (tp_in_vgpr: the player vectors are alike in every lane, and in scalar registers
// the descent spills)
__device__ __forceinline__ uint32_t ts_in_vgpr(const uint32_t x)
{
    uint32_t v;
    asm("v_mov_b32 %0, %1" : "=v"(v) : "s"(x));
    return v;
}

template <typename T>
__device__ __forceinline__ T *ts_ptr_in_vgpr(T *p)
{
    const uint64_t a = reinterpret_cast<uint64_t>(p);
    return reinterpret_cast<T *>(((uint64_t)ts_in_vgpr((uint32_t)(a >> 32)) << 32) | (uint64_t)ts_in_vgpr((uint32_t)a));
}

__device__ __forceinline__ uint32_t ts_eq01(const uint32_t a, const uint32_t b)
{
    const uint32_t x = a ^ b;
    return ((x | (0u - x)) >> 31) ^ 1u;
}

template <int P>
struct TsPos {
    int h[P], x[P], y[P], d[P], k[P];
};

template <int P>
__device__ __forceinline__ uint32_t ts_alive(const TsPos<P> &s)
{
    uint32_t alive = 0u;
#pragma unroll
    for (int p = 0; p < P; ++p) alive |= (s.k[p] == 0 ? 1u : 0u) << p;
    return alive;
}

__device__ __forceinline__ int ts_avoid_cell(const int N, const int hx, const int hy, const int dir)
{
    const int dd = dir & 3;
    const int nx = min(max(hx + (dd == 1) - (dd == 3), 0), N - 1);
    const int ny = min(max(hy + (dd == 2) - (dd == 0), 0), N - 1);
    return ny * N + nx;
}

// tp_avoid_codes: crl_tron_sample_avoid's rule for every live player on the pre-step byte board, under the avoid playout tag
// with the tree steps' third counter word
template <int P>
__device__ __forceinline__ void ts_avoid_codes(const int N, const int NN, const int8_t *bd, const TsPos<P> &s, const uint32_t gid,
                                               const uint32_t c, const uint32_t k0, const uint32_t k1, const uint64_t thr, int (&code)[P])
{
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int c_f = ts_avoid_cell(N, s.x[p], s.y[p], s.d[p]);
        const int c_r = ts_avoid_cell(N, s.x[p], s.y[p], s.d[p] + 1);
        const int c_l = ts_avoid_cell(N, s.x[p], s.y[p], s.d[p] + 3);
        CRL_BOUNDS_LT(c_f, NN, 124);
        CRL_BOUNDS_LT(c_r, NN, 124);
        CRL_BOUNDS_LT(c_l, NN, 124);
        (void)NN;
        const int o_f = bd[c_f] > 0, o_r = bd[c_r] > 0, o_l = bd[c_l] > 0;
        const philox_out wv = philox4x32_10(gid, c, TS_TREE_STEP, CRL_TAG_TRON_AVOID_PLAYOUT | (uint32_t)p, k0, k1);
        const uint32_t a3 = __umulhi(wv.w[1], 3u);
        const bool left_first = (wv.w[2] >> 31) != 0u;
        const bool first_free = (left_first ? o_l : o_r) == 0;
        const int side = (left_first == first_free) ? 3 : 1;
        const int a = ((uint64_t)wv.w[0] < thr) ? (int)(a3 + (a3 >> 1)) : (o_f == 0 ? 0 : side);
        code[p] = s.k[p] == 0 ? a : 0;
        __builtin_amdgcn_sched_barrier(0);                       // one player's block at a time, as in tron_puct.hip
    }
}

// tp_random_codes: crl_tron_rollout's digit rule with j = c & 7 under the random playout tag
template <int P>
__device__ __forceinline__ void ts_random_codes(const uint32_t gid, const uint32_t c, const uint32_t k0, const uint32_t k1, int (&code)[P])
{
    const uint32_t sel = (c & 7u) >> 1;
    const philox_out wa = philox4x32_10(gid, c >> 3, TS_TREE_STEP, CRL_TAG_TRON_PLAYOUT, k0, k1);
    const uint32_t word_a = sel == 0u ? wa.w[0] : sel == 1u ? wa.w[1] : sel == 2u ? wa.w[2] : wa.w[3];
    uint32_t word_b = 0u;
    if constexpr (P > 4) {
        const philox_out wb = philox4x32_10(gid, c >> 3, TS_TREE_STEP, CRL_TAG_TRON_PLAYOUT | 1u, k0, k1);
        word_b = sel == 0u ? wb.w[0] : sel == 1u ? wb.w[1] : sel == 2u ? wb.w[2] : wb.w[3];
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const uint32_t lo3 = (p & 3) == 0 ? 1u : (p & 3) == 1 ? 3u : (p & 3) == 2 ? 9u : 27u;
        const uint32_t v = (p < 4 ? word_a : word_b) * ((c & 1u) ? 81u * lo3 : lo3);
        const uint32_t a3 = __umulhi(v, 3u);
        code[p] = (int)(a3 + (a3 >> 1));
    }
}

// tp_step: crl_tron_step without reset on the byte board WITH OWNERS, in the reference's sequential order
template <int P>
__device__ __forceinline__ void ts_step(const int N, const int NN, int8_t *bd, TsPos<P> &s, const int (&code)[P])
{
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const bool run = s.k[i] == 0;
        const int dir = (s.d[i] + code[i]) & 3;
        s.d[i] = run ? dir : s.d[i];
        const int nx = s.x[i] + (dir == 1) - (dir == 3);
        const int ny = s.y[i] + (dir == 2) - (dir == 0);
        const bool oob = (unsigned)nx >= (unsigned)N || (unsigned)ny >= (unsigned)N;
        const int cell = oob ? s.h[i] : ny * N + nx;
        CRL_BOUNDS_LT(cell, NN, 125);
        (void)NN;
        const int val = bd[cell];
        const bool occupied = val > 0;
        const bool crash = run & !oob & occupied;
        const bool moved = run & !oob & !occupied;
        s.k[i] = run ? (oob ? i + 1 : (occupied ? val : 0)) : s.k[i];
        const uint32_t crashed = crash ? 1u : 0u;
#pragma unroll
        for (int o = 0; o < P; ++o) {
            const uint32_t hit = crashed & ts_eq01((uint32_t)val, (uint32_t)(o + 1)) & ts_eq01((uint32_t)s.h[o], (uint32_t)cell);
            s.k[o] += (int)hit * (i + 1 - s.k[o]);
        }
        bd[cell] = (int8_t)(moved ? i + 1 : val);
        s.h[i] = moved ? cell : s.h[i];
        s.x[i] = moved ? nx : s.x[i];
        s.y[i] = moved ? ny : s.y[i];
#pragma unroll
        for (int o = 0; o < P; ++o) asm volatile("" : "+v"(s.k[o]));
        asm volatile("" : "+v"(s.h[i]), "+v"(s.x[i]), "+v"(s.y[i]), "+v"(s.d[i]));
    }
}

// ---- the packed network (tron_net.hip states the layout) and this kernel's LDS
constexpr int TS_MIN_H = 16, TS_MAX_H = 256, TS_MAX_L = 3, TS_MAX_N = 40;
constexpr int TS_TREES = 16;
constexpr unsigned TS_MAX_BLOCKS = 512;                          // two workgroups a CU on 256 CUs, a grid-stride loop past that
constexpr int TS_ROOT_WORDS = 24;                                // a tree's 16 header words and 8 player words, staged once a group
// the per-leaf tables, int32 [16] each
constexpr int TS_M_HEAD = 0, TS_M_DIR = 1, TS_M_SEAT = 2, TS_M_NODES = 3, TS_M_SIMS = 4, TS_M_DEPTH = 5, TS_M_KIND = 6, TS_M_LEAF = 7,
              TS_M_LIVE = 8, TS_M_TABLES = 9;

struct ts_layout {
    uint32_t NN, NNp;           // cells, padded to a multiple of 16
    uint32_t K0;                // the first layer's padded inputs: 4 NNp + 16
    uint32_t hidden, head;      // floats: where the later layers and the head matrix start in the packed network
    uint32_t RS, AS;            // bytes of a board row (tn_layout's odd-quad stride), floats of an activation row
    // LDS, in bytes: the working boards at 0, then
    uint32_t o_root;            // the resident root boards, 16 rows of RS
    uint32_t o_act;             // two activation buffers of 16 x AS floats
    uint32_t o_out;             // float [16][4]: the logits of forward, right, left and the value
    uint32_t o_words;           // uint32 [16][TS_ROOT_WORDS]
    uint32_t o_meta;            // int32 [TS_M_TABLES][16]
    uint32_t o_flag;            // uint8 [2][16]: the pending flags, alternating by trip
    uint32_t lds;
};

__host__ __device__ inline ts_layout ts_layout_of(const int N, const int H, const int L)
{
    ts_layout y;
    const uint32_t h = (uint32_t)H;
    y.NN = (uint32_t)(N * N);
    y.NNp = ts_pad16(y.NN);
    y.K0 = 4u * y.NNp + 16u;
    y.hidden = h * y.K0 + h;
    y.head = y.hidden + (uint32_t)(L - 1) * (h * h + h);
    y.RS = y.NNp + (((y.NNp >> 4) & 1u) ? 0u : 16u);
    y.AS = h + 4u;
    y.o_root = TS_TREES * y.RS;
    y.o_act = y.o_root + TS_TREES * y.RS;
    y.o_out = y.o_act + 2u * TS_TREES * y.AS * 4u;
    y.o_words = y.o_out + TS_TREES * 16u;
    y.o_meta = y.o_words + TS_TREES * TS_ROOT_WORDS * 4u;
    y.o_flag = y.o_meta + TS_M_TABLES * TS_TREES * 4u;
    y.lds = y.o_flag + 2u * TS_TREES;                            // N = 5, H = 16: 6,496 bytes; N = 40, H = 256: 87,392
    return y;
}

__device__ __forceinline__ f32x4 ts_relu(const f32x4 v)
{
    f32x4 y;
    y.x = fmaxf(v.x, 0.0f), y.y = fmaxf(v.y, 0.0f), y.z = fmaxf(v.z, 0.0f), y.w = fmaxf(v.w, 0.0f);
    return y;
}

// tn_mac: acc += (the A fragments of one packed tile, this lane's float4 at w) x (the four inputs this lane holds)
__device__ __forceinline__ f32x4 ts_mac(const float *__restrict__ w, const f32x4 in, f32x4 acc)
{
    const f32x4 a = *reinterpret_cast<const f32x4 *>(w);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, in.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, in.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, in.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, in.w, acc, 0, 0, 0);
    return acc;
}

// the B values of one k tile of a board plane, from the ABSOLUTE ids against the seat's id s1 = seat + 1 (the head of this file)
template <int PLANE>
__device__ __forceinline__ f32x4 ts_plane_bits(const uint32_t word, const int cell0, const int head, const uint32_t s1)
{
    f32x4 x;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint32_t b = (word >> (8 * r)) & 255u;
        bool on;
        if constexpr (PLANE == 0) on = b == 0u;
        else if constexpr (PLANE == 1) on = b == s1;
        else if constexpr (PLANE == 2) on = b - 1u < 127u && b != s1;
        else on = cell0 + r == head;
        x[r] = on ? 1.0f : 0.0f;
    }
    return x;
}

// k tiles PLANE * CT .. + CT - 1 of output tile T of the first layer (wt: the tile's first packed kilobyte, this lane's float4)
template <int PLANE>
__device__ __forceinline__ f32x4 ts_first_plane(const float *__restrict__ wt, const uint8_t *brow, const int CT, const int g,
                                                const int head, const uint32_t s1, f32x4 acc)
{
    for (int ct = 0; ct < CT; ++ct) {
        const uint32_t word = PLANE < 3 ? *reinterpret_cast<const uint32_t *>(brow + 16 * ct + 4 * g) : 0u;
        acc = ts_mac(wt + (size_t)(PLANE * CT + ct) * 256, ts_plane_bits<PLANE>(word, 16 * ct + 4 * g, head, s1), acc);
    }
    return acc;
}

// ---- phase 2: the 16 working boards through the network; three logits and the value of every leaf into `out`.  The whole
// workgroup runs it (it holds barriers); wave `wave` of `waves` computes output tiles wave, wave + waves, ... of every layer.
__device__ __forceinline__ void ts_mlp(const ts_layout &lay, const int H, const int L, const float *__restrict__ net,
                                       const uint8_t *work, float *act0, float *out, const int *meta, const int wave, const int waves,
                                       const int lane)
{
    const int n = lane & 15, g = lane >> 4, HT = H >> 4, CT = (int)lay.NNp >> 4, KT0 = 4 * CT + 1, AS = (int)lay.AS;
    {
        const float *b0 = net + (size_t)H * lay.K0;
        const uint8_t *brow = work + n * (int)lay.RS;
        const int head = meta[TS_M_HEAD * TS_TREES + n], dir = meta[TS_M_DIR * TS_TREES + n];
        const uint32_t s1 = (uint32_t)meta[TS_M_SEAT * TS_TREES + n] + 1u;
        f32x4 face;
#pragma unroll
        for (int r = 0; r < 4; ++r) face[r] = (g == 0 && dir == r) ? 1.0f : 0.0f;
        for (int T = wave; T < HT; T += waves) {
            const float *wt = net + ((size_t)T * KT0 * 64 + lane) * 4;
            f32x4 acc = *reinterpret_cast<const f32x4 *>(b0 + 16 * T + 4 * g);
            acc = ts_first_plane<0>(wt, brow, CT, g, head, s1, acc);
            acc = ts_first_plane<1>(wt, brow, CT, g, head, s1, acc);
            acc = ts_first_plane<2>(wt, brow, CT, g, head, s1, acc);
            acc = ts_first_plane<3>(wt, brow, CT, g, head, s1, acc);
            acc = ts_mac(wt + (size_t)(4 * CT) * 256, face, acc);
            *reinterpret_cast<f32x4 *>(act0 + n * AS + 16 * T + 4 * g) = ts_relu(acc);
        }
        __syncthreads();
    }
    for (int l = 1; l < L; ++l) {
        const float *w = net + lay.hidden + (size_t)(l - 1) * (H * H + H), *b = w + H * H;
        const float *in = act0 + ((l - 1) & 1) * TS_TREES * AS + n * AS + 4 * g;
        float *o = act0 + (l & 1) * TS_TREES * AS + n * AS + 4 * g;
        for (int T = wave; T < HT; T += waves) {
            f32x4 acc = *reinterpret_cast<const f32x4 *>(b + 16 * T + 4 * g);
            for (int t = 0; t < HT; ++t)
                acc = ts_mac(w + ((size_t)(T * HT + t) * 64 + lane) * 4, *reinterpret_cast<const f32x4 *>(in + 16 * t), acc);
            *reinterpret_cast<f32x4 *>(o + 16 * T) = ts_relu(acc);
        }
        __syncthreads();
    }
    if (wave == 0) {                                             // the head tile: lane n < 16 holds (forward, right, left, value) of leaf n
        const float *w = net + lay.head, *b = w + 16 * H;
        const float *in = act0 + ((L - 1) & 1) * TS_TREES * AS + n * AS + 4 * g;
        f32x4 y = *reinterpret_cast<const f32x4 *>(b + 4 * g);
        for (int t = 0; t < HT; ++t)
            y = ts_mac(w + ((size_t)t * 64 + lane) * 4, *reinterpret_cast<const f32x4 *>(in + 16 * t), y);
        if (g == 0) *reinterpret_cast<f32x4 *>(out + 4 * n) = y;
    }
    __syncthreads();
}

// ---- phase 1: tron_puct_select_kernel's descent of the tree in slot `slot`, statement for statement, on the slot's working
// board; the leaf's head, facing and pending flag into the tables.  The header is written once a simulation, by ts_backup.
template <int P>
__device__ __forceinline__ void ts_descend(const int N, const int NN, const uint32_t inv_n, const ts_tree &t, const int S_cap,
                                           const uint32_t cpuct, const uint32_t fpu, const int lane, const int slot, const int nchunks,
                                           uint8_t *bd_u, const uint8_t *root, const uint32_t *words, int *meta, uint8_t *flag)
{
    int8_t *const bd = reinterpret_cast<int8_t *>(bd_u);
    uint32_t nn = (uint32_t)__builtin_amdgcn_readfirstlane(meta[TS_M_NODES * TS_TREES + slot]);
    const uint32_t sims = (uint32_t)__builtin_amdgcn_readfirstlane(meta[TS_M_SIMS * TS_TREES + slot]);
    const bool live = __builtin_amdgcn_readfirstlane(meta[TS_M_LIVE * TS_TREES + slot]) != 0;
    const int sp = min(__builtin_amdgcn_readfirstlane(meta[TS_M_SEAT * TS_TREES + slot]), P - 1);
    bool pend = false, went = false;
    int d = 0, term = 0, seat_alive = 1, leaf = 0, hs = 0, ds = 0;
    if (live && sims < (uint32_t)S_cap) {                        // (a skipped or a full tree is left alone)
        went = true;
        // ---- the reset: the resident root board onto the working board, lanes over 16-byte chunks
        for (int j = lane; j < nchunks; j += 64) reinterpret_cast<uint4 *>(bd_u)[j] = reinterpret_cast<const uint4 *>(root)[j];
        TsPos<P> ps;
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const uint32_t pw = ts_in_vgpr((uint32_t)__builtin_amdgcn_readfirstlane((int)words[16 + p]));
            ps.h[p] = min((int)(pw & 0xffffu), NN - 1);
            ps.y[p] = (int)__umulhi((uint32_t)ps.h[p], inv_n);
            ps.x[p] = ps.h[p] - ps.y[p] * N;
            ps.d[p] = (int)((pw >> 16) & 3u);
            ps.k[p] = (int)(int8_t)(pw >> 24);
        }
        const uint32_t tc = ts_in_vgpr((uint32_t)__builtin_amdgcn_readfirstlane((int)words[TS_H_TCOUNT]));
        const uint32_t gid = ts_in_vgpr((uint32_t)__builtin_amdgcn_readfirstlane((int)words[TS_H_GID]));
        const uint32_t k0 = ts_in_vgpr((uint32_t)__builtin_amdgcn_readfirstlane((int)words[TS_H_SEED_LO]));
        const uint32_t k1 = ts_in_vgpr((uint32_t)__builtin_amdgcn_readfirstlane((int)words[TS_H_SEED_HI]));
        const bool avoid = __builtin_amdgcn_readfirstlane((int)words[TS_H_MODEL]) != 0;
        const uint64_t thr = ((uint64_t)words[TS_H_THR_HI] << 32) | (uint64_t)words[TS_H_THR_LO];
        uint32_t is_seat[P];
#pragma unroll
        for (int p = 0; p < P; ++p) is_seat[p] = ts_in_vgpr(p == sp ? 1u : 0u);
        ts_wave_sync();
        int v = 0;
        for (;;) {
            CRL_BOUNDS_LT(v, S_cap + 1, 126);
            const uint32_t nv = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.n[v]);
            if (nv == 0u) { pend = true; leaf = v; break; }     // an unexpanded node: the pending leaf
            if (d >= S_cap) break;                               // (never: a path of d edges has d + 1 distinct nodes)
            // ---- lane a scores the child at action a
            const size_t at = (size_t)v * 3u + (size_t)(lane < 3 ? lane : 0);
            const uint32_t pe = lane < 3 ? t.prior[at] : 0u;
            uint32_t cu = lane < 3 ? t.child[at] : 0u;
            CRL_BOUNDS_LT(cu, S_cap + 1, 127);
            cu = min(cu, (uint32_t)S_cap);
            const uint64_t rt = ts_isqrt((uint64_t)min(nv, 4095u) << 16);
            uint32_t key = 0u;
            if (lane < 3) {
                const uint32_t nu = cu ? min(t.n[cu], 4095u) : 0u, wu = cu ? t.w[cu] : 0u;
                const uint64_t exploit = nu ? ts_div(wu, nu) : (uint64_t)fpu;
                const uint64_t explore = ts_div((uint64_t)cpuct * pe * rt, (1u + nu) << 16);
                key = (uint32_t)min(exploit + explore, (uint64_t)0x7fffffffu);
            }
            const uint32_t key0 = (uint32_t)__builtin_amdgcn_readlane((int)key, 0), key1 = (uint32_t)__builtin_amdgcn_readlane((int)key, 1),
                           key2 = (uint32_t)__builtin_amdgcn_readlane((int)key, 2);
            const int e = key1 > key0 ? (key2 > key1 ? 2 : 1) : (key2 > key0 ? 2 : 0);
            const int c0 = __builtin_amdgcn_readlane((int)cu, 0), c1 = __builtin_amdgcn_readlane((int)cu, 1),
                      c2 = __builtin_amdgcn_readlane((int)cu, 2);
            int u = e == 0 ? c0 : e == 1 ? c1 : c2;
            const bool fresh = u == 0;
            if (fresh) {
                if (nn > (uint32_t)S_cap) break;                 // (never: nodes <= simulations + 1 <= S_cap)
                u = (int)nn++;
                CRL_BOUNDS_LT(u, S_cap + 1, 128);
                if (lane == e) t.child[at] = (uint16_t)u;
                if (lane < 3) { t.prior[(size_t)u * 3u + lane] = 0; t.child[(size_t)u * 3u + lane] = 0; }
                if (lane == 0) { t.n[u] = 0u; t.w[u] = 0u; }
            }
            // ---- the tree step at depth d: the seat plays e, the others the model agent on the pre-step position
            int code[P];
            const uint32_t c = tc + (uint32_t)d;
            if (avoid) {
                ts_avoid_codes<P>(N, NN, bd, ps, gid, c, k0, k1, thr, code);
            } else {
                ts_random_codes<P>(gid, c, k0, k1, code);
            }
#pragma unroll
            for (int p = 0; p < P; ++p) code[p] += (int)is_seat[p] * (e + (e >> 1) - code[p]);
            ts_step<P>(N, NN, bd, ps, code);
            d += 1;
            CRL_BOUNDS_LT(d, S_cap + 1, 129);
            if (lane == 0) t.path[d] = (uint16_t)u;
            const uint32_t alive = ts_alive<P>(ps);
            seat_alive = __builtin_amdgcn_readfirstlane((int)((alive >> sp) & 1u));
            term = (!seat_alive || __builtin_amdgcn_readfirstlane(__popc(alive)) <= 1) ? 1 : 0;   // CLOSED, crl_tron_mcts's rule
            leaf = u;
            if (term) break;
            if (fresh) { pend = true; break; }                   // the new node is the leaf: nothing of it is read back
            v = u;
        }
        if (lane == 0) t.path[0] = 0;
#pragma unroll
        for (int p = 0; p < P; ++p) { hs = is_seat[p] ? ps.h[p] : hs; ds = is_seat[p] ? ps.d[p] : ds; }
    }
    if (lane == 0) {
        meta[TS_M_HEAD * TS_TREES + slot] = hs;                  // (what select hands out as row 0 of obs_heads / obs_dirs)
        meta[TS_M_DIR * TS_TREES + slot] = ds & 3;
        meta[TS_M_NODES * TS_TREES + slot] = (int)nn;
        meta[TS_M_DEPTH * TS_TREES + slot] = d;
        meta[TS_M_KIND * TS_TREES + slot] = (went ? 4 : 0) | (pend ? 1 : 0) | (term ? 2 : 0) | (seat_alive << 8);
        meta[TS_M_LEAF * TS_TREES + slot] = leaf;
        *flag = pend ? 1 : 0;
    }
}

// ---- phase 3: tron_net_eval_kernel's epilogue and tron_puct_backup_kernel for the tree in slot `slot`, then the header words
// select and backup leave behind
__device__ __forceinline__ void ts_backup(const ts_tree &t, const int S_cap, const int lane, const int slot, int *meta, const float *out)
{
    const int kind = __builtin_amdgcn_readfirstlane(meta[TS_M_KIND * TS_TREES + slot]);
    if ((kind & 4) == 0) return;                                 // not descended: skipped, at capacity or a missing row
    const bool pend = (kind & 1) != 0, have = (kind & 3) != 0;
    const int d = __builtin_amdgcn_readfirstlane(meta[TS_M_DEPTH * TS_TREES + slot]);
    const uint32_t nn = (uint32_t)__builtin_amdgcn_readfirstlane(meta[TS_M_NODES * TS_TREES + slot]);
    uint32_t sims = (uint32_t)__builtin_amdgcn_readfirstlane(meta[TS_M_SIMS * TS_TREES + slot]);
    const uint32_t seat_alive = ((uint32_t)kind >> 8) & 1u;
    if (have) {
        const int plen = d + 1;
        uint32_t add = seat_alive ? 65536u : 0u;                 // a terminal leaf: the seat alive or not
        if (pend) {
            const int lf = __builtin_amdgcn_readfirstlane(meta[TS_M_LEAF * TS_TREES + slot]);
            CRL_BOUNDS_LT(lf, S_cap + 1, 126);
            const uint32_t Lf = min((uint32_t)lf, (uint32_t)S_cap);
            const f32x4 y = *reinterpret_cast<const f32x4 *>(out + 4 * slot);
            const float top = fmaxf(fmaxf(y.x, y.y), y.z);
            const float la = lane == 0 ? y.x : (lane == 1 ? y.y : y.z);
            const float e = 65535.0f * expf(la - top);
            const uint32_t pr = lane < 3 ? (uint32_t)(uint16_t)min(max(__float2int_rn(e), 0), 65535) : 0u;   // (NaN: 0)
            const float s = 65536.0f / (1.0f + expf(-y.w));
            const int value = min(max(__float2int_rn(s), 0), 65536);
            const uint32_t sum = (uint32_t)__builtin_amdgcn_readlane((int)pr, 0) + (uint32_t)__builtin_amdgcn_readlane((int)pr, 1) +
                                 (uint32_t)__builtin_amdgcn_readlane((int)pr, 2);
            const uint32_t share = (uint32_t)min((uint64_t)65535u, sum ? ts_div((uint64_t)pr << 16, max(sum, 1u)) : (uint64_t)(65536u / 3u));
            if (lane < 3) t.prior[(size_t)Lf * 3u + lane] = (uint16_t)share;
            add = (uint32_t)min(max(value, 0), 65536);
        }
        for (int i0 = 0; i0 < plen; i0 += 64) {                  // lane i adds to the node at depth i (distinct nodes: no atomics)
            const int i = i0 + lane;
            if (i < plen) {
                CRL_BOUNDS_LT(t.path[i], S_cap + 1, 127);
                const uint32_t node = min((uint32_t)t.path[i], (uint32_t)S_cap);
                t.n[node] += 1u;
                if (i > 0) t.w[node] += add;
            }
        }
        sims += 1u;
    }
    if (lane == 0) {
        t.hdr[TS_H_NODES] = nn;
        t.hdr[TS_H_SIMS] = sims;
        t.hdr[TS_H_PATH] = 0u;
        t.hdr[TS_H_LEAF] = (pend ? TS_PENDING : TS_TERMINAL) | (seat_alive << 8);
        meta[TS_M_SIMS * TS_TREES + slot] = (int)sims;
    }
}

template <int P, int WAVES>
__global__ void __launch_bounds__(64 * WAVES)
tron_puct_search_kernel(const int N, const uint32_t inv_n, const int64_t B, uint8_t *trees_arg, const uint64_t tree_bytes,
                        const int S_cap, const int n_sims, const uint32_t cpuct, const uint32_t fpu, const float *__restrict__ net,
                        const ts_layout lay, const int H, const int L)
{
    constexpr int TPW = TS_TREES / WAVES;                        // trees a wave
    extern __shared__ __attribute__((aligned(16))) uint8_t ts_lds[];
    uint8_t *const work = ts_lds, *const root = ts_lds + lay.o_root;
    float *const act0 = reinterpret_cast<float *>(ts_lds + lay.o_act), *const out = reinterpret_cast<float *>(ts_lds + lay.o_out);
    uint32_t *const words = reinterpret_cast<uint32_t *>(ts_lds + lay.o_words);
    int *const meta = reinterpret_cast<int *>(ts_lds + lay.o_meta);
    uint8_t *const flags = ts_lds + lay.o_flag;
    uint8_t *const trees = ts_ptr_in_vgpr(trees_arg);            // (and so do a tree's array pointers, as in select)
    const int lane = (int)(threadIdx.x & 63u), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int NN = (int)lay.NN, RS = (int)lay.RS, nchunks = (int)lay.NNp >> 4;

    const int64_t groups = (B + TS_TREES - 1) / TS_TREES;
    uint32_t trip = 0;                                           // the flags alternate between two sets: a wave may be a phase ahead
    for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        __syncthreads();                                         // the last group's MLP has read the boards and the tables
        // ---- once a group: the header and player words, the root board (the bytes behind N N: no feature) and the tables
#pragma unroll 1
        for (int k = 0; k < TPW; ++k) {
            const int slot = wave * TPW + k;
            const int64_t b = grp * TS_TREES + slot;
            const bool row = b < B;                              // a missing row of a ragged group: no tree is touched
            const ts_tree t = ts_tree_of(trees, row ? b : 0, tree_bytes, S_cap, NN);
            const uint32_t nn = row ? (uint32_t)__builtin_amdgcn_readfirstlane((int)t.hdr[TS_H_NODES]) : 0u;
            const uint32_t sims = row ? (uint32_t)__builtin_amdgcn_readfirstlane((int)t.hdr[TS_H_SIMS]) : 0u;
            const bool live = nn != 0u && nn <= (uint32_t)S_cap + 1u;
            if (lane < TS_ROOT_WORDS) words[slot * TS_ROOT_WORDS + lane] = live ? t.hdr[lane] : 0u;   // (players: hdr + 16)
            for (int j = lane; j < nchunks; j += 64)
                reinterpret_cast<uint4 *>(root + slot * RS)[j] = live ? reinterpret_cast<const uint4 *>(t.board)[j] : make_uint4(0u, 0u, 0u, 0u);
            if (!live)                                           // a row nobody descends: an empty board under the MLP of the others
                for (int j = lane; j < nchunks; j += 64) reinterpret_cast<uint4 *>(work + slot * RS)[j] = make_uint4(0u, 0u, 0u, 0u);
            if (lane < TS_M_TABLES) {
                int m = 0;
                m = lane == TS_M_SEAT ? (live ? (int)(t.hdr[TS_H_SEAT] & 7u) : 0) : m;
                m = lane == TS_M_NODES ? (int)nn : m;
                m = lane == TS_M_SIMS ? (int)sims : m;
                m = lane == TS_M_LIVE ? (live ? 1 : 0) : m;
                meta[lane * TS_TREES + slot] = m;
            }
            if (live && sims >= (uint32_t)S_cap && lane == 0) t.hdr[TS_H_PATH] = 0u;   // at capacity: no path (select's word)
            ts_wave_sync();
            if (lane < (int)lay.NNp - NN) root[slot * RS + NN + lane] = 255;
        }
        ts_wave_sync();
        for (int s = 0; s < n_sims; ++s, ++trip) {
            uint8_t *flag = flags + TS_TREES * (trip & 1u);
#pragma unroll 1
            for (int k = 0; k < TPW; ++k) {
                const int slot = wave * TPW + k;
                const int64_t b = grp * TS_TREES + slot;
                ts_descend<P>(N, NN, inv_n, ts_tree_of(trees, b < B ? b : 0, tree_bytes, S_cap, NN), S_cap, cpuct, fpu, lane, slot, nchunks,
                              work + slot * RS, root + slot * RS, words + slot * TS_ROOT_WORDS, meta, flag + slot);
            }
            __syncthreads();
            if (__ballot(lane < TS_TREES && flag[lane & (TS_TREES - 1)] != 0) != 0ull)   // (alike in every wave)
                ts_mlp(lay, H, L, net, work, act0, out, meta, wave, WAVES, lane);
#pragma unroll 1
            for (int k = 0; k < TPW; ++k) {
                const int slot = wave * TPW + k;
                const int64_t b = grp * TS_TREES + slot;
                ts_backup(ts_tree_of(trees, b < B ? b : 0, tree_bytes, S_cap, NN), S_cap, lane, slot, meta, out);
            }
            ts_wave_sync();                                      // the next descent reads what these lanes stored
        }
    }
}

// the geometry of a player count: 16 waves of one tree where the instance fits 128 VGPRs without scratch, else 8 waves of two.
// As compiled the 16-wave instances of EVERY player count spill (P = 1: 2 VGPRs, 12 bytes of scratch a lane; P = 4: 29 and 120),
// so all eight run as 8 waves of two trees (profiles/tron_puct_search_kernel_stats.txt)
constexpr int ts_waves_of(const int P) { return P >= 1 ? 8 : 16; }

template <int P>
int ts_launch(const unsigned blocks, const ts_layout &lay, hipStream_t st, const int N, const uint32_t inv_n, const int64_t B,
              uint8_t *trees, const uint64_t tree_bytes, const int S_cap, const int n_sims, const uint32_t cpuct, const uint32_t fpu,
              const float *net, const int H, const int L)
{
    const auto kernel = tron_puct_search_kernel<P, ts_waves_of(P)>;
    if (lay.lds > 64u * 1024u)                                   // (more than 64 KB of dynamic LDS is an opt-in)
        CRL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lay.lds));
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64u * ts_waves_of(P)), lay.lds, st, N, inv_n, B, trees, tree_bytes, S_cap, n_sims,
                       cpuct, fpu, net, lay, H, L);
    return CRL_OK;
}

} // namespace

int crl_tron_puct_search_bounds(unsigned int *out4)
{
    CRL_BOUNDS_READBACK(out4);
    return CRL_OK;
}

extern "C" {

int crl_tron_puct_search(const crl_ctx *ctx, int64_t B, void *tree, int S_cap, int n_sims, const void *net, int H, int L,
                         uint32_t cpuct, uint32_t fpu, uint32_t flags, void *stream)
{
    TRON_CTX_CHECK("crl_tron_puct_search");
    CRL_REQUIRE(tree != nullptr, "crl_tron_puct_search: NULL tree pointer");
    CRL_REQUIRE((((uintptr_t)tree) & 15) == 0, "crl_tron_puct_search: tree must be 16-byte aligned");
    CRL_REQUIRE(S_cap >= 1 && S_cap <= TS_MAX_S, "crl_tron_puct_search: S_cap=%d out of range 1..%d", S_cap, TS_MAX_S);
    CRL_REQUIRE(n_sims >= 1 && n_sims <= TS_MAX_S, "crl_tron_puct_search: n_sims=%d out of range 1..%d", n_sims, TS_MAX_S);
    CRL_REQUIRE(H >= TS_MIN_H && H <= TS_MAX_H && H % 16 == 0, "crl_tron_puct_search: H=%d is not a multiple of 16 in %d..%d", H,
                TS_MIN_H, TS_MAX_H);
    CRL_REQUIRE(L >= 1 && L <= TS_MAX_L, "crl_tron_puct_search: L=%d out of range 1..%d", L, TS_MAX_L);
    CRL_REQUIRE(net != nullptr, "crl_tron_puct_search: NULL net pointer");
    CRL_REQUIRE((((uintptr_t)net) & 15) == 0, "crl_tron_puct_search: net must be 16-byte aligned");
    CRL_REQUIRE(cpuct <= 65535u, "crl_tron_puct_search: cpuct=%u out of range 0..65535", cpuct);
    CRL_REQUIRE(fpu <= 65536u, "crl_tron_puct_search: fpu=%u out of range 0..65536", fpu);
    CRL_REQUIRE(flags == 0, "crl_tron_puct_search: unknown flags 0x%x", flags);
    const crl_tron_cfg &cfg = ctx->tron;
    if (cfg.N > TS_MAX_N) {
        crl_set_error("crl_tron_puct_search: N=%d: boards above %dx%d do not fit the kernel's LDS plan", cfg.N, TS_MAX_N, TS_MAX_N);
        return CRL_EUNSUPPORTED;
    }
    const int NN = cfg.N * cfg.N;
    const uint64_t tree_bytes = ts_tree_bytes(S_cap, NN);
    const ts_layout lay = ts_layout_of(cfg.N, H, L);
    const uint32_t inv_n = (uint32_t)(0x100000000ull / (uint32_t)cfg.N) + 1u;   // y = umulhi(h, inv_n) is exact for h < N*N <= 2^15
    const uint64_t groups = ((uint64_t)B + TS_TREES - 1u) / TS_TREES;
    const unsigned blocks = (unsigned)(groups < TS_MAX_BLOCKS ? groups : TS_MAX_BLOCKS);
    int rc = CRL_OK;
    TRON_DISPATCH_P(cfg.P, rc = (ts_launch<PP>(blocks, lay, (hipStream_t)stream, cfg.N, inv_n, B, static_cast<uint8_t *>(tree), tree_bytes,
                                               S_cap, n_sims, cpuct, fpu, static_cast<const float *>(net), H, L)));
    if (rc != CRL_OK) return rc;
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

} // extern "C"
