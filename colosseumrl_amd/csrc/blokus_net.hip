// blokus_net.hip -- the policy-value MLP between crl_blokus_puct_select and crl_blokus_puct_backup in one launch
// (crl_blokus_net_*; the contract is in include/colosseum_hip.h), gfx950, wave64, float32 MFMA (v_mfma_f32_16x16x4_f32).
// DESIGN.md 4.5q states the layout below with the measurements.  The trunk is tron_net.hip's: a WORKGROUP of four waves owns 16
// leaves per trip and computes the transposed chain Y^T = W X^T, the weight tile the A operand (16 outputs x 4 inputs), the
// activations the B operand (4 inputs x 16 leaves); with n = lane % 16 and g = lane / 16 the accumulator of output tile T
// holds, in lane (n, g), outputs 16 T + 4 g + r (r = 0..3) of leaf n, and k-step (t, r) contracts over input 16 t + 4 g + r.
// The output tiles of every layer are dealt over the waves (wave w computes tiles w, w + 4, ...).  What is Blokus's own:
//
// THE POLICY HEAD SCORES A LIST.  A leaf carries up to W <= 64 sampled candidates out of 336,000 ids, so the head does not emit
// a vector over the actions: it emits a MAP q over the 400 observation cells and a term r per piece, and the logit of a
// candidate is r[piece] plus q over the cells the candidate would cover.  The head is ONE packed matrix of 425 rows padded to
// 432 (27 output tiles: cells 0..399, pieces 400..420, value 421..424), dealt over the waves like a hidden layer, four tiles
// in flight per wave; its results go to LDS, not to registers.  Then, behind a barrier, the CANDIDATE PHASE: each wave takes
// four leaves of the tile in turn, one lane per candidate slot -- decode the id (constant divisions), fetch the oriented
// offsets (8 bytes out of the staged cell table), rotate each cell into the mover's frame, gather up to five q and one r from
// the map, wave-reduce the maximum, exp, store.
//
// LDS of a workgroup (dynamic; the host computes the same map)
//   map      16 rows of BNET_MS = 436 floats: the head's 432 outputs of each leaf (436 / 4 is odd: the 16 rows of a fragment
//            fall on 16 different bank quads).  It LIES OVER the staged inputs, which are dead behind layer 1:
//     boards   16 rows of 400 bytes (400 / 16 is odd), the rows of a ragged last tile -1 (no feature)
//     pieces   16 rows of 112 bytes: the 84 inventory bytes as 4 (held) or 255, 255 behind them (the piece k tiles read 96)
//   act[2]   16 rows of H + 4 floats each: layer l reads act[(l - 1) & 1] and writes act[l & 1]
//   tab      the first 1,368 bytes of the context's BlkTables: cells[168][8] and ncell[24]
//   mover, K, pend   int32 [16] each: mover & 3, clamp(n_cand, 0, W), pending
// H = 256: 27,904 + 33,280 + 1,376 + 192 = 62,752 bytes.
// One barrier before the inputs are overwritten (the last trip's map reads are over), one behind the load, one behind every
// hidden layer, one behind the head.
//
// The packed network (net_pack), in floats: every matrix in TILE ORDER -- [output tile T][k tile t][lane][r] holds
// W[16 T + lane % 16][16 t + 4 (lane / 16) + r], the A fragments of a (T, t) tile ONE coalesced kilobyte -- each followed by
// its bias.  The first matrix has K0 = 1,696 columns: the four owner planes of 400 columns are whole k tiles already (25 a
// plane), the 84 piece columns follow at 1,600 as they do in the feature vector and are padded with 12 zero columns.  So a
// lane's four B values of a board k tile are four byte compares of one LDS word against the plane's constant, those of a
// piece tile four compares against 4 (an inventory byte is staged as 4 or 255); no division in the k loop, and the products
// are exact.
//
// THE ORDER OF EVERY SUM is a function of (H, L) alone (never of B, W, the grid, the wave that runs it or timing): an output
// starts from its bias and adds one MFMA k-step after the other, k tiles ascending, within a k tile r = 0, 1, 2, 3, each step
// the hardware's sum over the four inputs 16 t + r + {0, 4, 8, 12}; a logit starts from r[piece] and adds its cells in table
// order.  No sum is split over waves or lanes.
#define BLK_DEVICE_ONLY
#include "blokus.hip"
#include <stddef.h>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int BNET_MIN_H = 16, BNET_MAX_H = 256, BNET_MAX_L = 3, BNET_MATS = BNET_MAX_L + 3;
constexpr int BNET_WAVES = 4;                                     // waves of a workgroup: one a SIMD
constexpr unsigned BNET_MAX_BLOCKS = 1024;                        // four workgroups a CU on 256 CUs, a grid-stride loop past that
constexpr int BNET_CELLS = BN * BN, BNET_F = 4 * BNET_CELLS + 4 * NPIECE;            // 400 cells, 1,684 features
constexpr int BNET_PT = 6, BNET_KT0 = 4 * (BNET_CELLS / 16) + BNET_PT, BNET_K0 = 16 * BNET_KT0;   // 6 piece k tiles; 106 k tiles, 1,696 columns
constexpr int BNET_HEAD_PIECE = BNET_CELLS, BNET_HEAD_VALUE = BNET_CELLS + NPIECE;   // rows 400.. and 421.. of the head matrix
constexpr int BNET_HEAD_ROWS = BNET_HEAD_VALUE + 4, BNET_HEAD_TILES = (BNET_HEAD_ROWS + 15) / 16, BNET_HEAD_PAD = 16 * BNET_HEAD_TILES;
constexpr int BNET_RS = BNET_CELLS, BNET_PS = 112, BNET_MS = BNET_HEAD_PAD + 4;      // LDS strides: board bytes, piece bytes, map floats
constexpr int BNET_MAP_BYTES = 16 * BNET_MS * 4;
constexpr int BNET_TAB_BYTES = NSHAPE * 8 + 24, BNET_TAB_PAD = (BNET_TAB_BYTES + 15) & ~15;
static_assert(BNET_CELLS % 16 == 0 && BNET_HEAD_TILES == 27 && BNET_K0 == 1696, "the k tiles of a plane and the head's tiles");
static_assert(16 * BNET_RS + 16 * BNET_PS <= BNET_MAP_BYTES && 16 * BNET_PT <= BNET_PS, "the staged inputs lie under the map");
static_assert(offsetof(BlkTables, cells) == 0 && offsetof(BlkTables, ncell) == NSHAPE * 8, "the staged front of BlkTables");

// where the parts of a packed network and of the LDS lie (host and device agree on it here and nowhere else)
struct bnet_layout {
    uint32_t hidden;            // floats: the first of the L - 1 layers H x H, each H * H + H floats
    uint32_t head;              // floats: the head matrix 432 x H, then its 432 biases
    uint32_t total;             // floats
    uint32_t AS;                // LDS: floats of an activation row
    uint32_t lds;               // bytes of LDS
};

__host__ __device__ inline bnet_layout bnet_layout_of(const int H, const int L)
{
    bnet_layout y;
    const uint32_t h = (uint32_t)H;
    y.hidden = h * (uint32_t)BNET_K0 + h;
    y.head = y.hidden + (uint32_t)(L - 1) * (h * h + h);
    y.total = y.head + (uint32_t)BNET_HEAD_PAD * h + (uint32_t)BNET_HEAD_PAD;          // H = 256, L = 3: 677,040 floats
    y.AS = h + 4u;
    y.lds = (uint32_t)BNET_MAP_BYTES + 2u * 16u * y.AS * 4u + (uint32_t)BNET_TAB_PAD + 3u * 16u * 4u;   // H = 256: 62,752 bytes
    return y;
}

// ---- pack: every element of the packed buffer from its place in the caller's matrices, zeros in the padding
struct bnet_pack_args {
    const float *w[BNET_MATS], *b[BNET_MATS];
    int L, H;
};

// element `at` of a matrix in tile order with `cols` padded columns -> (row, col) of the padded row-major matrix
__device__ __forceinline__ void bnet_tile_rc(const uint32_t at, const uint32_t cols, uint32_t &row, uint32_t &col)
{
    const uint32_t T = at / (cols * 16u), rem = at - T * cols * 16u, t = rem >> 8, lane = (rem >> 2) & 63u, r = rem & 3u;
    row = 16u * T + (lane & 15u);
    col = 16u * t + 4u * (lane >> 4) + r;
}

// row `row` of the head matrix: which of the caller's three heads (0 cells, 1 pieces, 2 value) and which of its rows; false: padding
__device__ __forceinline__ bool bnet_head_row(const uint32_t row, uint32_t &which, uint32_t &sub)
{
    if (row < (uint32_t)BNET_HEAD_PIECE) { which = 0u; sub = row; return true; }
    if (row < (uint32_t)BNET_HEAD_VALUE) { which = 1u; sub = row - (uint32_t)BNET_HEAD_PIECE; return true; }
    if (row < (uint32_t)BNET_HEAD_ROWS) { which = 2u; sub = row - (uint32_t)BNET_HEAD_VALUE; return true; }
    return false;
}

__global__ void __launch_bounds__(256)
blokus_net_pack_kernel(const bnet_pack_args a, const bnet_layout lay, float *__restrict__ net)
{
    const uint32_t H = (uint32_t)a.H, L = (uint32_t)a.L;
    for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < lay.total; e += gridDim.x * 256u) {
        float v = 0.0f;
        uint32_t row, col, which, sub;
        if (e < lay.hidden) {                                     // the first layer: [H, 1684], twelve zero columns behind it
            if (e < H * (uint32_t)BNET_K0) {
                bnet_tile_rc(e, (uint32_t)BNET_K0, row, col);
                if (col < (uint32_t)BNET_F) v = a.w[0][(size_t)row * BNET_F + col];
            } else {
                v = a.b[0][e - H * (uint32_t)BNET_K0];
            }
        } else if (e < lay.head) {                                // hidden layer l = 1 .. L - 1: [H, H]
            const uint32_t per = H * H + H, l = 1u + (e - lay.hidden) / per, at = (e - lay.hidden) - (l - 1u) * per;
            if (at < H * H) {
                bnet_tile_rc(at, H, row, col);
                v = a.w[l][(size_t)row * H + col];
            } else {
                v = a.b[l][at - H * H];
            }
        } else {                                                  // the three heads as one matrix of 432 rows
            const uint32_t at = e - lay.head;
            if (at < (uint32_t)BNET_HEAD_PAD * H) {
                bnet_tile_rc(at, H, row, col);
                if (bnet_head_row(row, which, sub)) v = a.w[L + which][(size_t)sub * H + col];
            } else if (bnet_head_row(at - (uint32_t)BNET_HEAD_PAD * H, which, sub)) {
                v = a.b[L + which][sub];
            }
        }
        net[e] = v;
    }
}

// ---- eval
__device__ __forceinline__ f32x4 bnet_relu(const f32x4 v)
{
    f32x4 y;
    y.x = fmaxf(v.x, 0.0f), y.y = fmaxf(v.y, 0.0f), y.z = fmaxf(v.z, 0.0f), y.w = fmaxf(v.w, 0.0f);
    return y;
}

// acc += (the A fragments of one packed tile, this lane's float4 a) x (the four inputs this lane holds): four k-steps
__device__ __forceinline__ f32x4 bnet_mac(const f32x4 a, const f32x4 in, f32x4 acc)
{
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, in.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, in.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, in.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, in.w, acc, 0, 0, 0);
    return acc;
}

// A CHUNK of N consecutive k tiles t0 .. t0 + N - 1 of a layer of KT k tiles, whose B values are x[0 .. N - 1], into the
// output tiles first, first + 4, ... (those below `tiles`; NT accumulators).  All N NT weight fragments are fetched before the
// first MFMA, so one trip to memory is paid per chunk and not per tile (a workgroup's LDS leaves room for two or three waves
// a SIMD: nothing else hides it); the k loops around a chunk are not unrolled.  Per accumulator the k tiles stay ascending.
template <int NT, int N>
__device__ __forceinline__ void bnet_chunk(const float *__restrict__ w, const int KT, const int t0, const int tiles, const int first,
                                           const int lane, const f32x4 (&x)[N], f32x4 (&acc)[NT])
{
    f32x4 a[NT][N];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int T = min(first + BNET_WAVES * j, tiles - 1);
#pragma unroll
        for (int u = 0; u < N; ++u) a[j][u] = *reinterpret_cast<const f32x4 *>(w + ((size_t)(T * KT + t0 + u) * 64 + lane) * 4);
    }
#pragma unroll
    for (int u = 0; u < N; ++u) {
#pragma unroll
        for (int j = 0; j < NT; ++j)
            if (first + BNET_WAVES * j < tiles) acc[j] = bnet_mac(a[j][u], x[u], acc[j]);
    }
}

// a chunk of the first layer: the B values of k tile t0 + u are four byte compares of the LDS word at bytes + 16 u against
// `is` -- a board plane's owner 0..3 (own, next, across, previous; -1, the empty cell, and any other byte set none), or 4 for
// the inventory bytes, which are staged as 4 (held) or 255
template <int TPW, int N>
__device__ __forceinline__ void bnet_first_chunk(const float *__restrict__ w0, const uint8_t *__restrict__ bytes, const uint32_t is,
                                                 const int t0, const int HT, const int wave, const int lane, f32x4 (&acc)[TPW])
{
    f32x4 x[N];
#pragma unroll
    for (int u = 0; u < N; ++u) {
        const uint32_t word = *reinterpret_cast<const uint32_t *>(bytes + 16 * u);
#pragma unroll
        for (int r = 0; r < 4; ++r) x[u][r] = ((word >> (8 * r)) & 255u) == is ? 1.0f : 0.0f;
    }
    bnet_chunk<TPW, N>(w0, BNET_KT0, t0, HT, wave, lane, x, acc);
}

// NT output tiles first, first + 4, ... (those below `tiles`) of a layer of KT k tiles over the activations at `in`
template <int NT>
__device__ __forceinline__ void bnet_dense(const float *__restrict__ w, const float *__restrict__ b, const float *__restrict__ in,
                                           const int KT, const int tiles, const int first, const int lane, const int g,
                                           f32x4 (&acc)[NT])
{
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = *reinterpret_cast<const f32x4 *>(b + 16 * min(first + BNET_WAVES * j, tiles - 1) + 4 * g);
    int t = 0;
#pragma unroll 1
    for (; t + 4 <= KT; t += 4) {
        f32x4 x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = *reinterpret_cast<const f32x4 *>(in + 16 * (t + u));
        bnet_chunk<NT, 4>(w, KT, t, tiles, first, lane, x, acc);
    }
#pragma unroll 1
    for (; t < KT; ++t) {                                         // H not a multiple of 64
        f32x4 x[1];
        x[0] = *reinterpret_cast<const f32x4 *>(in + 16 * t);
        bnet_chunk<NT, 1>(w, KT, t, tiles, first, lane, x, acc);
    }
}

__device__ __forceinline__ float bnet_wave_max(float v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = fmaxf(v, __shfl_xor(v, s, 64));
    return v;
}

// TPW: output tiles of a hidden layer per wave = ceil(H / 16 / 4).  Two waves a SIMD is what the LDS of H >= 192 leaves room
// for (three up to 176), and TPW = 3 is held to the registers of two; TPW = 4 (H >= 208) would spill there and runs one workgroup a CU.
template <int TPW>
__global__ void __launch_bounds__(64 * BNET_WAVES) __attribute__((amdgpu_waves_per_eu(TPW < 4 ? 2 : 1)))
blokus_net_eval_kernel(const bnet_layout lay, const int H, const int L, const int W, const int64_t B, const float *__restrict__ net,
                       const uint32_t *__restrict__ tables, const int8_t *__restrict__ board, const uint8_t *__restrict__ pieces,
                       const int32_t *__restrict__ cand, const int32_t *__restrict__ n_cand, const int8_t *__restrict__ mover,
                       const uint8_t *__restrict__ pending, uint16_t *__restrict__ prior, int32_t *__restrict__ value)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t bnet_lds[];
    const int AS = (int)lay.AS;
    uint8_t *const boards = bnet_lds, *const invs = bnet_lds + 16 * BNET_RS;
    float *const map = reinterpret_cast<float *>(bnet_lds);
    float *const act0 = reinterpret_cast<float *>(bnet_lds + BNET_MAP_BYTES);
    uint8_t *const tab = reinterpret_cast<uint8_t *>(act0 + 2 * 16 * AS);
    int *const mover_of = reinterpret_cast<int *>(tab + BNET_TAB_PAD), *const k_of = mover_of + 16, *const pend_of = k_of + 16;
    const int tid = (int)threadIdx.x, lane = tid & 63, n = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: the weight tiles are addressed from SGPRs
    const int HT = H >> 4;
    for (int i = tid; i < BNET_TAB_BYTES / 4; i += 64 * BNET_WAVES) reinterpret_cast<uint32_t *>(tab)[i] = tables[i];
    const int64_t tiles = (B + 15) >> 4;
    for (int64_t tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
        const int64_t leaf = tl * 16 + n;
        const bool pend = leaf < B && (pending == nullptr || pending[leaf] != 0);
        const int rows_here = (int)min((int64_t)16, B - tl * 16);
        if (__ballot(pend) == 0ull) {                            // the same 16 bytes in every wave: the whole workgroup skips
            for (int i = tid; i < rows_here * W; i += 64 * BNET_WAVES) prior[tl * 16 * W + i] = 0;
            if (tid < rows_here * 4) value[tl * 64 + tid] = 0;
            continue;
        }
        __syncthreads();                                         // the last trip's reads of the map and the activations are over
        {
            const int8_t *src = board + tl * 16 * BNET_CELLS;
            for (int c = tid; c < 16 * BNET_RS; c += 64 * BNET_WAVES)
                boards[c] = c < rows_here * BNET_CELLS ? (uint8_t)src[c] : (uint8_t)255;
            const uint8_t *inv = pieces + tl * 16 * (4 * NPIECE);
            for (int c = tid; c < 16 * BNET_PS; c += 64 * BNET_WAVES) {
                const int r = c / BNET_PS, i = c - r * BNET_PS;
                invs[c] = (r < rows_here && i < 4 * NPIECE && inv[r * (4 * NPIECE) + i] != 0) ? (uint8_t)4 : (uint8_t)255;
            }
        }
        if (tid < 16) {
            const bool have = tid < rows_here;
            mover_of[tid] = have ? ((int)mover[tl * 16 + tid] & 3) : 0;
            k_of[tid] = have ? min(max(n_cand[tl * 16 + tid], 0), W) : 0;
            pend_of[tid] = (have && (pending == nullptr || pending[tl * 16 + tid] != 0)) ? 1 : 0;
        }
        __syncthreads();

        // ---- the first layer: the four owner planes, then the piece tiles; its B operand is made here from the staged bytes
        f32x4 acc[TPW];
        {
            const float *w0 = net, *b0 = net + (size_t)H * BNET_K0;
#pragma unroll
            for (int j = 0; j < TPW; ++j) {
                const int T = min(wave + BNET_WAVES * j, HT - 1);
                acc[j] = *reinterpret_cast<const f32x4 *>(b0 + 16 * T + 4 * g);
            }
            const uint8_t *brow = boards + n * BNET_RS + 4 * g;
            constexpr int CT = BNET_CELLS / 16;
            static_assert(CT % 5 == 0, "a plane's k tiles in chunks of five");
#pragma unroll 1
            for (int plane = 0; plane < 4; ++plane) {
#pragma unroll 1
                for (int ct = 0; ct < CT; ct += 5)
                    bnet_first_chunk<TPW, 5>(w0, brow + 16 * ct, (uint32_t)plane, plane * CT + ct, HT, wave, lane, acc);
            }
            bnet_first_chunk<TPW, BNET_PT>(w0, invs + n * BNET_PS + 4 * g, 4u, 4 * CT, HT, wave, lane, acc);
#pragma unroll
            for (int j = 0; j < TPW; ++j) {
                const int T = wave + BNET_WAVES * j;
                if (T < HT) *reinterpret_cast<f32x4 *>(act0 + n * AS + 16 * T + 4 * g) = bnet_relu(acc[j]);
            }
        }
        __syncthreads();

        // ---- the hidden layers: act[(l - 1) & 1] -> act[l & 1]
        for (int l = 1; l < L; ++l) {
            const float *w = net + lay.hidden + (size_t)(l - 1) * (H * H + H);
            float *out = act0 + (l & 1) * 16 * AS + n * AS + 4 * g;
            bnet_dense<TPW>(w, w + H * H, act0 + ((l - 1) & 1) * 16 * AS + n * AS + 4 * g, HT, HT, wave, lane, g, acc);
#pragma unroll
            for (int j = 0; j < TPW; ++j) {
                const int T = wave + BNET_WAVES * j;
                if (T < HT) *reinterpret_cast<f32x4 *>(out + 16 * T) = bnet_relu(acc[j]);
            }
            __syncthreads();
        }

        // ---- the head: 27 output tiles over the waves, four in flight, into the map (over the boards, dead since layer 1)
        {
            const float *w = net + lay.head;
            const float *in = act0 + ((L - 1) & 1) * 16 * AS + n * AS + 4 * g;
#pragma unroll 1
            for (int first = wave; first < BNET_HEAD_TILES; first += 4 * BNET_WAVES) {
                f32x4 y[4];
                bnet_dense<4>(w, w + (size_t)BNET_HEAD_PAD * H, in, HT, BNET_HEAD_TILES, first, lane, g, y);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int T = first + BNET_WAVES * j;
                    if (T < BNET_HEAD_TILES) *reinterpret_cast<f32x4 *>(map + n * BNET_MS + 16 * T + 4 * g) = y[j];
                }
            }
        }
        __syncthreads();

        // ---- the candidates: wave w takes leaves 4 w .. 4 w + 3 of the tile in turn, lane k the candidate slot k
#pragma unroll 1
        for (int q = 0; q < 4; ++q) {
            const int row = 4 * wave + q;
            const int64_t lf = tl * 16 + row;
            if (lf >= B) break;
            const float *mrow = map + row * BNET_MS;
            const bool pd = pend_of[row] != 0;
            const int K = k_of[row], m = mover_of[row];
            CRL_BOUNDS_IN(K, 0, W + 1, 390);
            const bool have = pd && lane < K;
            float l = 0.0f;
            if (have) {
                const int id = cand[lf * W + lane];
                if (id >= 0 && id < ACTION_IDS) {
                    const BlkMove mv = blk_decode(id);
                    const int shape = min(mv.piece * 8 + mv.orient, NSHAPE - 1);
                    CRL_BOUNDS_IN(mv.piece, 0, NPIECE, 391);
                    const int nc = (int)tab[NSHAPE * 8 + mv.piece];
                    if (mv.shift < nc) {
                        const uint2 cw = *reinterpret_cast<const uint2 *>(tab + 8 * shape);
                        const uint64_t cells = (uint64_t)cw.x | ((uint64_t)cw.y << 32);
                        const int oc = (int)((cells >> (8 * mv.shift)) & 255u);
                        l = mrow[BNET_HEAD_PIECE + mv.piece];
#pragma unroll
                        for (int j = 0; j < 5; ++j) {
                            const int cc = (int)((cells >> (8 * j)) & 255u);
                            const int X = mv.x + (cc & 15) - (oc & 15), Y = mv.y + (cc >> 4) - (oc >> 4);
                            if (j < nc && (unsigned)X < (unsigned)BN && (unsigned)Y < (unsigned)BN) {
                                const int a = (m & 1) ? X : Y, b = (m & 1) ? Y : X;                       // the inverse of blk_write_observation's rotation
                                const int oi = (m & 2) ? BN - 1 - a : a, oj = (m == 1 || m == 2) ? BN - 1 - b : b;
                                const int cell = min(max(BN * oi + oj, 0), BNET_CELLS - 1);
                                CRL_BOUNDS_IN(BN * oi + oj, 0, BNET_CELLS, 392);
                                l += mrow[cell];
                            }
                        }
                    }
                }
            }
            const float top = bnet_wave_max(have ? l : -INFINITY);
            if (lane < W) {
                const float e = have ? 65535.0f * expf(l - top) : 0.0f;
                prior[lf * W + lane] = (uint16_t)min(max(__float2int_rn(e), 0), 65535);                  // (NaN: 0)
            }
            if (lane < 4) {
                const float s = pd ? 65536.0f / (1.0f + expf(-mrow[BNET_HEAD_VALUE + lane])) : 0.0f;
                value[lf * 4 + lane] = min(max(__float2int_rn(s), 0), 65536);
            }
        }
    }
}

// (the context is checked last, as in the other Blokus entries: every other refusal can be had without a device)
#define BNET_REQUIRE_CTX(fn)                                                                                                   \
    CRL_REQUIRE(ctx != nullptr && ctx->game == CRL_GAME_BLOKUS && ctx->blokus, "%s: ctx is not a blokus context", fn)

#define BNET_REQUIRE_SHAPE(fn)                                                                                                 \
    CRL_REQUIRE(H >= BNET_MIN_H && H <= BNET_MAX_H && H % 16 == 0, "%s: H=%d is not a multiple of 16 in %d..%d", fn, H,        \
                BNET_MIN_H, BNET_MAX_H);                                                                                       \
    CRL_REQUIRE(L >= 1 && L <= BNET_MAX_L, "%s: L=%d out of range 1..%d", fn, L, BNET_MAX_L)

#define BNET_REQUIRE_BUFFER(fn)                                                                                                \
    CRL_REQUIRE(net != nullptr, "%s: NULL net pointer", fn);                                                                   \
    CRL_REQUIRE((((uintptr_t)net) & 15) == 0, "%s: net must be 16-byte aligned", fn)

} // namespace

// {failures, first code, first value, first limit} of this translation unit's bounds asserts (codes 390..399)
int crl_blokus_net_bounds(unsigned int *out4)
{
    CRL_BOUNDS_READBACK(out4);
    return CRL_OK;
}

extern "C" {

int64_t crl_blokus_net_bytes(const crl_ctx *ctx, int H, int L)
{
    BNET_REQUIRE_SHAPE("crl_blokus_net_bytes");
    BNET_REQUIRE_CTX("crl_blokus_net_bytes");
    return (int64_t)bnet_layout_of(H, L).total * 4;
}

int crl_blokus_net_pack(const crl_ctx *ctx, int H, int L, const float *const *weight, const float *const *bias, void *net,
                        void *stream)
{
    BNET_REQUIRE_SHAPE("crl_blokus_net_pack");
    BNET_REQUIRE_BUFFER("crl_blokus_net_pack");
    CRL_REQUIRE(weight != nullptr && bias != nullptr, "crl_blokus_net_pack: NULL weight or bias array");
    for (int s = 0; s < L + 3; ++s)
        CRL_REQUIRE(weight[s] != nullptr && bias[s] != nullptr, "crl_blokus_net_pack: NULL weight or bias pointer of matrix %d", s);
    BNET_REQUIRE_CTX("crl_blokus_net_pack");
    const bnet_layout lay = bnet_layout_of(H, L);
    bnet_pack_args a = {};
    a.L = L, a.H = H;
    for (int s = 0; s < L + 3; ++s) a.w[s] = weight[s], a.b[s] = bias[s];
    const unsigned want = (lay.total + 255u) / 256u;
    hipLaunchKernelGGL(blokus_net_pack_kernel, dim3(want < 4096u ? want : 4096u), dim3(256), 0, (hipStream_t)stream, a, lay,
                       static_cast<float *>(net));
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

#define BNET_EVAL_CASE(TPW_)                                                                                                   \
    case TPW_:                                                                                                                 \
        hipLaunchKernelGGL(blokus_net_eval_kernel<TPW_>, dim3(blocks), dim3(64 * BNET_WAVES), lay.lds, (hipStream_t)stream, lay, H, \
                           L, W, B, static_cast<const float *>(net), static_cast<const uint32_t *>(ctx->blokus), obs_board,    \
                           obs_pieces, cand, n_cand, mover, pending, prior, value);                                            \
        break

int crl_blokus_net_eval(const crl_ctx *ctx, int64_t B, const void *net, int H, int L, int W, const int8_t *obs_board,
                        const uint8_t *obs_pieces, const int32_t *cand, const int32_t *n_cand, const int8_t *mover,
                        const uint8_t *pending, uint16_t *prior, int32_t *value, uint32_t flags, void *stream)
{
    BNET_REQUIRE_SHAPE("crl_blokus_net_eval");
    CRL_REQUIRE(W >= 1 && W <= 64, "crl_blokus_net_eval: W=%d out of range 1..64", W);
    CRL_REQUIRE(B > 0 && B <= ((int64_t)1 << 31), "crl_blokus_net_eval: B=%lld out of range", (long long)B);
    BNET_REQUIRE_BUFFER("crl_blokus_net_eval");
    CRL_REQUIRE(obs_board && obs_pieces && cand && n_cand && mover, "crl_blokus_net_eval: NULL input pointer");
    CRL_REQUIRE(prior && value, "crl_blokus_net_eval: NULL output pointer");
    CRL_REQUIRE(flags == 0, "crl_blokus_net_eval: unknown flags 0x%x", flags);
    BNET_REQUIRE_CTX("crl_blokus_net_eval");
    const bnet_layout lay = bnet_layout_of(H, L);
    const uint64_t tiles = ((uint64_t)B + 15u) / 16u;
    const unsigned blocks = (unsigned)(tiles < BNET_MAX_BLOCKS ? tiles : BNET_MAX_BLOCKS);
    switch ((H / 16 + BNET_WAVES - 1) / BNET_WAVES) {
        BNET_EVAL_CASE(1); BNET_EVAL_CASE(2); BNET_EVAL_CASE(3); BNET_EVAL_CASE(4);
    }
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

} // extern "C"
