// tron_net.hip -- the policy-value MLP between crl_tron_puct_select and crl_tron_puct_backup in one launch (crl_tron_net_*; the
// contract is in include/colosseum_hip.h), gfx950, wave64, float32 MFMA (v_mfma_f32_16x16x4_f32).  DESIGN.md 4.5o states the
// layout below with the measurements.
//
// A WORKGROUP of four waves (one a SIMD) owns 16 leaves per trip and computes the transposed chain Y^T = W X^T of ttt_net.hip:
// the weight tile is the A operand (16 outputs x 4 inputs), the activations are the B operand (4 inputs x 16 leaves).  With
// n = lane % 16 and g = lane / 16 the accumulator of output tile T holds, in lane (n, g), outputs 16 T + 4 g + r (r = 0..3) of
// leaf n, and k-step (t, r) contracts over input 16 t + 4 g + r.  The first layer has F = 4 N N + 4 inputs (1,604 at 20x20):
// one wave would run every output tile's k loop alone, so the OUTPUT TILES of every layer are dealt over the waves (wave w
// computes tiles w, w + 4, ...: at most four accumulators) and the activations pass between the layers through LDS.
//
// LDS of a workgroup (dynamic; the host computes the same map)
//   boards   16 rows of RS bytes: the 16 observed boards, RS = pad16(N N), plus 16 where that makes RS / 16 odd, so that the
//            16 rows of a fragment fall on 16 different bank quads; the bytes behind N N and the rows of a ragged last tile
//            are -1 (no feature)
//   act[2]   16 rows of H + 4 floats each (the same odd-quad padding): layer l reads act[(l - 1) & 1] and writes act[l & 1]
//   head, dir  int32 [16] each: the seat's head cell clamped onto the board, its facing & 3
// One barrier before the boards are overwritten, one behind the load, one behind every hidden layer.
//
// The packed network (net_pack), in floats: every matrix in TILE ORDER -- [output tile T][k tile t][lane][r] holds
// W[16 T + lane % 16][16 t + 4 (lane / 16) + r], so the A fragments of a (T, t) tile are ONE coalesced kilobyte and a wave's k
// loop streams consecutive kilobytes -- each followed by its bias.  The first matrix's columns are regrouped: each of the four
// planes (empty, own, other, head) is padded with zero columns to pad16(N N), the four facing columns are a k tile of their
// own (4 + 12 zeros), so every k tile lies in one plane and a lane's four B values are four byte compares of one LDS word
// against a constant -- no division in the k loop; the products are exact.  The three policy rows and the value row are ONE
// matrix of 16 rows (policy 0..2, value 3, zeros): one head tile, computed by wave 0, whose lanes 0..15 then hold the three
// logits and the value of their leaf -- the epilogue needs no cross-lane move.
//
// THE ORDER OF EVERY SUM is a function of (N, H, L) alone (never of B, the grid, the wave that runs it or timing): an output
// starts from its bias and adds one MFMA k-step after the other, k tiles ascending in packed order (plane 0's cells ascending,
// planes 1, 2, 3, the facing tile; then inputs ascending in the later layers), within a k tile r = 0, 1, 2, 3, each step the
// hardware's sum over the four inputs 16 t + r + {0, 4, 8, 12}.  No sum is split over waves.
#include "crl_common.hpp"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TN_MIN_H = 16, TN_MAX_H = 256, TN_MAX_L = 3, TN_MATS = TN_MAX_L + 2;
constexpr int TN_WAVES = 4;                                       // waves of a workgroup: one a SIMD
constexpr int TN_MAX_N = 40;                                      // 16 boards of N N bytes beside the activations in 64 KB of LDS
constexpr unsigned TN_MAX_BLOCKS = 1024;                          // four workgroups a CU on 256 CUs, a grid-stride loop past that

__host__ __device__ inline uint32_t tn_pad16(const uint32_t x) { return (x + 15u) & ~15u; }

// where the parts of a packed network and of the LDS lie (host and device agree on it here and nowhere else)
struct tn_layout {
    uint32_t NN, NNp;           // cells, padded to a multiple of 16
    uint32_t K0;                // the first layer's padded inputs: 4 NNp + 16
    uint32_t hidden;            // floats: the first of the L - 1 layers H x H, each H * H + H floats
    uint32_t head;              // floats: the head matrix 16 x H, then its 16 biases
    uint32_t total;             // floats
    uint32_t RS, AS;            // LDS: bytes of a board row, floats of an activation row
    uint32_t lds;               // bytes of LDS
};

__host__ __device__ inline tn_layout tn_layout_of(const int N, const int H, const int L)
{
    tn_layout y;
    const uint32_t h = (uint32_t)H;
    y.NN = (uint32_t)(N * N);
    y.NNp = tn_pad16(y.NN);
    y.K0 = 4u * y.NNp + 16u;
    y.hidden = h * y.K0 + h;
    y.head = y.hidden + (uint32_t)(L - 1) * (h * h + h);
    y.total = y.head + 16u * h + 16u;                             // N <= 40: < 2^21 floats
    y.RS = y.NNp + (((y.NNp >> 4) & 1u) ? 0u : 16u);
    y.AS = h + 4u;
    y.lds = 16u * y.RS + 2u * 16u * y.AS * 4u + 2u * 16u * 4u;     // N = 40, H = 256: 59,264 bytes
    return y;
}

// ---- pack: every element of the packed buffer from its place in the caller's matrices, zeros in the padding
struct tn_pack_args {
    const float *w[TN_MATS], *b[TN_MATS];
    int L, H;
};

// element `at` of a matrix in tile order with `cols` padded columns -> (row, col) of the padded row-major matrix
__device__ __forceinline__ void tn_tile_rc(const uint32_t at, const uint32_t cols, uint32_t &row, uint32_t &col)
{
    const uint32_t T = at / (cols * 16u), rem = at - T * cols * 16u, t = rem >> 8, lane = (rem >> 2) & 63u, r = rem & 3u;
    row = 16u * T + (lane & 15u);
    col = 16u * t + 4u * (lane >> 4) + r;
}

__global__ void __launch_bounds__(256)
tron_net_pack_kernel(const tn_pack_args a, const tn_layout lay, float *__restrict__ net)
{
    const uint32_t H = (uint32_t)a.H, L = (uint32_t)a.L;
    for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < lay.total; e += gridDim.x * 256u) {
        float v = 0.0f;
        uint32_t row, col;
        if (e < lay.hidden) {                                     // the first layer: [H, 4 N N + 4] behind the regrouped columns
            if (e < H * lay.K0) {
                tn_tile_rc(e, lay.K0, row, col);
                const uint32_t plane = col / lay.NNp, cell = col - plane * lay.NNp;
                if (plane < 4u) {
                    if (cell < lay.NN) v = a.w[0][(size_t)row * (4u * lay.NN + 4u) + plane * lay.NN + cell];
                } else if (cell < 4u) {
                    v = a.w[0][(size_t)row * (4u * lay.NN + 4u) + 4u * lay.NN + cell];
                }
            } else {
                v = a.b[0][e - H * lay.K0];
            }
        } else if (e < lay.head) {                                // hidden layer l = 1 .. L - 1: [H, H]
            const uint32_t per = H * H + H, l = 1u + (e - lay.hidden) / per, at = (e - lay.hidden) - (l - 1u) * per;
            if (at < H * H) {
                tn_tile_rc(at, H, row, col);
                v = a.w[l][(size_t)row * H + col];
            } else {
                v = a.b[l][at - H * H];
            }
        } else {                                                  // the heads as one tile: policy rows 0..2, the value row 3
            const uint32_t at = e - lay.head;
            if (at < 16u * H) {
                tn_tile_rc(at, H, row, col);
                if (row < 3u) v = a.w[L][(size_t)row * H + col];
                else if (row == 3u) v = a.w[L + 1u][col];
            } else {
                row = at - 16u * H;
                if (row < 3u) v = a.b[L][row];
                else if (row == 3u) v = a.b[L + 1u][0];
            }
        }
        net[e] = v;
    }
}

// ---- eval
__device__ __forceinline__ f32x4 tn_relu(const f32x4 v)
{
    f32x4 y;
    y.x = fmaxf(v.x, 0.0f), y.y = fmaxf(v.y, 0.0f), y.z = fmaxf(v.z, 0.0f), y.w = fmaxf(v.w, 0.0f);
    return y;
}

// acc += (the A fragments of one packed tile, this lane's float4 at w) x (the four inputs this lane holds): four k-steps
__device__ __forceinline__ f32x4 tn_mac(const float *__restrict__ w, const f32x4 in, f32x4 acc)
{
    const f32x4 a = *reinterpret_cast<const f32x4 *>(w);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, in.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, in.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, in.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, in.w, acc, 0, 0, 0);
    return acc;
}

// the B values of one k tile of a board plane: PLANE 0 empty, 1 the seat's own trail, 2 anybody else's, 3 the seat's head
template <int PLANE>
__device__ __forceinline__ f32x4 tn_plane_bits(const uint32_t word, const int cell0, const int head)
{
    f32x4 x;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint32_t b = (word >> (8 * r)) & 255u;
        bool on;
        if constexpr (PLANE == 0) on = b == 0u;
        else if constexpr (PLANE == 1) on = b == 1u;
        else if constexpr (PLANE == 2) on = b - 2u < 126u;        // (int8) > 1
        else on = cell0 + r == head;
        x[r] = on ? 1.0f : 0.0f;
    }
    return x;
}

// one plane of the first layer: k tiles PLANE * CT .. + CT - 1 into the wave's TPW accumulators
template <int PLANE, int TPW>
__device__ __forceinline__ void tn_first_plane(const float *__restrict__ w0, const uint8_t *__restrict__ brow, const int CT,
                                               const int KT0, const int HT, const int wave, const int lane, const int g,
                                               const int head, f32x4 (&acc)[TPW])
{
    for (int ct = 0; ct < CT; ++ct) {
        const uint32_t word = PLANE < 3 ? *reinterpret_cast<const uint32_t *>(brow + 16 * ct + 4 * g) : 0u;
        const f32x4 x = tn_plane_bits<PLANE>(word, 16 * ct + 4 * g, head);
        const int t = PLANE * CT + ct;
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
            const int T = wave + TN_WAVES * j;
            if (T < HT) acc[j] = tn_mac(w0 + ((size_t)(T * KT0 + t) * 64 + lane) * 4, x, acc[j]);
        }
    }
}

// TPW: output tiles of a layer per wave = ceil(H / 16 / 4)
template <int TPW>
__global__ void __launch_bounds__(64 * TN_WAVES)
tron_net_eval_kernel(const tn_layout lay, const int H, const int L, const int64_t B, const float *__restrict__ net,
                     const int8_t *__restrict__ board, const int16_t *__restrict__ heads, const int8_t *__restrict__ dirs,
                     const uint8_t *__restrict__ pending, uint16_t *__restrict__ prior, int32_t *__restrict__ value)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t tn_lds[];
    const int RS = (int)lay.RS, AS = (int)lay.AS, NN = (int)lay.NN, NNp = (int)lay.NNp;
    uint8_t *const boards = tn_lds;
    float *const act0 = reinterpret_cast<float *>(tn_lds + 16 * RS);
    int *const head_of = reinterpret_cast<int *>(act0 + 2 * 16 * AS), *const dir_of = head_of + 16;
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 15, g = lane >> 4;
    const int HT = H >> 4, CT = NNp >> 4, KT0 = 4 * CT + 1;
    const int64_t tiles = (B + 15) >> 4;
    for (int64_t tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
        const int64_t leaf = tl * 16 + n;
        const bool row = leaf < B;
        const bool pend = row && (pending == nullptr || pending[leaf] != 0);
        const int rows_here = (int)min((int64_t)16, B - tl * 16);
        if (__ballot(pend) == 0ull) {                            // the same 16 bytes in every wave: the whole workgroup skips
            if (tid < rows_here * 3) prior[tl * 48 + tid] = 0;
            if (tid < rows_here) value[tl * 16 + tid] = 0;
            continue;
        }
        __syncthreads();                                         // the last trip's reads of the boards and activations are over
        for (int r = 0; r < 16; ++r) {
            const int8_t *src = board + (tl * 16 + r) * NN;
            for (int c = tid; c < NNp; c += 64 * TN_WAVES)
                boards[r * RS + c] = (r < rows_here && c < NN) ? (uint8_t)src[c] : (uint8_t)255;
        }
        if (tid < 16) {
            const bool have = tl * 16 + tid < B;
            head_of[tid] = have ? min(max((int)heads[tl * 16 + tid], 0), NN - 1) : 0;
            dir_of[tid] = have ? ((int)dirs[tl * 16 + tid] & 3) : 0;
        }
        __syncthreads();

        // ---- the first layer: the planes in turn, then the facing tile; its B operand is made here from the board bytes
        f32x4 acc[TPW];
        {
            const float *w0 = net, *b0 = net + (size_t)H * lay.K0;
#pragma unroll
            for (int j = 0; j < TPW; ++j) {
                const int T = min(wave + TN_WAVES * j, HT - 1);
                acc[j] = *reinterpret_cast<const f32x4 *>(b0 + 16 * T + 4 * g);
            }
            const uint8_t *brow = boards + n * RS;
            const int head = head_of[n];
            tn_first_plane<0, TPW>(w0, brow, CT, KT0, HT, wave, lane, g, head, acc);
            tn_first_plane<1, TPW>(w0, brow, CT, KT0, HT, wave, lane, g, head, acc);
            tn_first_plane<2, TPW>(w0, brow, CT, KT0, HT, wave, lane, g, head, acc);
            tn_first_plane<3, TPW>(w0, brow, CT, KT0, HT, wave, lane, g, head, acc);
            f32x4 face;
#pragma unroll
            for (int r = 0; r < 4; ++r) face[r] = (g == 0 && dir_of[n] == r) ? 1.0f : 0.0f;
#pragma unroll
            for (int j = 0; j < TPW; ++j) {
                const int T = wave + TN_WAVES * j;
                if (T < HT) {
                    acc[j] = tn_mac(w0 + ((size_t)(T * KT0 + 4 * CT) * 64 + lane) * 4, face, acc[j]);
                    *reinterpret_cast<f32x4 *>(act0 + n * AS + 16 * T + 4 * g) = tn_relu(acc[j]);
                }
            }
        }
        __syncthreads();

        // ---- the hidden layers: act[(l - 1) & 1] -> act[l & 1]
        for (int l = 1; l < L; ++l) {
            const float *w = net + lay.hidden + (size_t)(l - 1) * (H * H + H), *b = w + H * H;
            const float *in = act0 + ((l - 1) & 1) * 16 * AS + n * AS + 4 * g;
            float *out = act0 + (l & 1) * 16 * AS + n * AS + 4 * g;
#pragma unroll
            for (int j = 0; j < TPW; ++j) {
                const int T = min(wave + TN_WAVES * j, HT - 1);
                acc[j] = *reinterpret_cast<const f32x4 *>(b + 16 * T + 4 * g);
            }
            for (int t = 0; t < HT; ++t) {
                const f32x4 x = *reinterpret_cast<const f32x4 *>(in + 16 * t);
#pragma unroll
                for (int j = 0; j < TPW; ++j) {
                    const int T = wave + TN_WAVES * j;
                    if (T < HT) acc[j] = tn_mac(w + ((size_t)(T * HT + t) * 64 + lane) * 4, x, acc[j]);
                }
            }
#pragma unroll
            for (int j = 0; j < TPW; ++j) {
                const int T = wave + TN_WAVES * j;
                if (T < HT) *reinterpret_cast<f32x4 *>(out + 16 * T) = tn_relu(acc[j]);
            }
            __syncthreads();
        }

        // ---- the head tile and the epilogue, wave 0: lane n < 16 holds (forward, right, left, value) of leaf n
        if (wave == 0) {
            const float *w = net + lay.head, *b = w + 16 * H;
            const float *in = act0 + ((L - 1) & 1) * 16 * AS + n * AS + 4 * g;
            f32x4 y = *reinterpret_cast<const f32x4 *>(b + 4 * g);
            for (int t = 0; t < HT; ++t)
                y = tn_mac(w + ((size_t)t * 64 + lane) * 4, *reinterpret_cast<const f32x4 *>(in + 16 * t), y);
            if (g == 0 && row) {
                const float top = fmaxf(fmaxf(y.x, y.y), y.z);
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const float e = pend ? 65535.0f * expf(y[a] - top) : 0.0f;
                    prior[leaf * 3 + a] = (uint16_t)min(max(__float2int_rn(e), 0), 65535);                 // (NaN: 0)
                }
                const float s = pend ? 65536.0f / (1.0f + expf(-y.w)) : 0.0f;
                value[leaf] = min(max(__float2int_rn(s), 0), 65536);
            }
        }
    }
}

#define TN_REQUIRE_SHAPE(fn)                                                                                                   \
    CRL_REQUIRE(ctx != nullptr && ctx->game == CRL_GAME_TRON, "%s: ctx is not a tron context", fn);                            \
    CRL_REQUIRE(H >= TN_MIN_H && H <= TN_MAX_H && H % 16 == 0, "%s: H=%d is not a multiple of 16 in %d..%d", fn, H, TN_MIN_H,  \
                TN_MAX_H);                                                                                                     \
    CRL_REQUIRE(L >= 1 && L <= TN_MAX_L, "%s: L=%d out of range 1..%d", fn, L, TN_MAX_L);                                      \
    if (ctx->tron.N > TN_MAX_N) {                                                                                              \
        crl_set_error("%s: N=%d: boards above %dx%d do not fit the kernel's LDS plan", fn, ctx->tron.N, TN_MAX_N, TN_MAX_N);   \
        return CRL_EUNSUPPORTED;                                                                                               \
    }

#define TN_REQUIRE_BUFFER(fn)                                                                                                  \
    CRL_REQUIRE(net != nullptr, "%s: NULL net pointer", fn);                                                                   \
    CRL_REQUIRE((((uintptr_t)net) & 15) == 0, "%s: net must be 16-byte aligned", fn)

} // namespace

extern "C" {

int64_t crl_tron_net_bytes(const crl_ctx *ctx, int H, int L)
{
    TN_REQUIRE_SHAPE("crl_tron_net_bytes");
    return (int64_t)tn_layout_of(ctx->tron.N, H, L).total * 4;
}

int crl_tron_net_pack(const crl_ctx *ctx, int H, int L, const float *const *weight, const float *const *bias, void *net,
                      void *stream)
{
    TN_REQUIRE_SHAPE("crl_tron_net_pack");
    TN_REQUIRE_BUFFER("crl_tron_net_pack");
    CRL_REQUIRE(weight != nullptr && bias != nullptr, "crl_tron_net_pack: NULL weight or bias array");
    for (int s = 0; s < L + 2; ++s)
        CRL_REQUIRE(weight[s] != nullptr && bias[s] != nullptr, "crl_tron_net_pack: NULL weight or bias pointer of matrix %d", s);
    const tn_layout lay = tn_layout_of(ctx->tron.N, H, L);
    tn_pack_args a = {};
    a.L = L, a.H = H;
    for (int s = 0; s < L + 2; ++s) a.w[s] = weight[s], a.b[s] = bias[s];
    const unsigned want = (lay.total + 255u) / 256u;
    hipLaunchKernelGGL(tron_net_pack_kernel, dim3(want < 4096u ? want : 4096u), dim3(256), 0, (hipStream_t)stream, a, lay,
                       static_cast<float *>(net));
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

#define TN_EVAL_CASE(TPW_)                                                                                                     \
    case TPW_:                                                                                                                 \
        hipLaunchKernelGGL(tron_net_eval_kernel<TPW_>, dim3(blocks), dim3(64 * TN_WAVES), lay.lds, (hipStream_t)stream, lay, H, L, B, \
                           static_cast<const float *>(net), obs_board, obs_heads, obs_dirs, pending, prior, value);            \
        break

int crl_tron_net_eval(const crl_ctx *ctx, int64_t B, const void *net, int H, int L, const int8_t *obs_board,
                      const int16_t *obs_heads, const int8_t *obs_dirs, const uint8_t *pending, uint16_t *prior, int32_t *value,
                      uint32_t flags, void *stream)
{
    TN_REQUIRE_SHAPE("crl_tron_net_eval");
    CRL_REQUIRE(B > 0 && B <= ((int64_t)1 << 31), "crl_tron_net_eval: B=%lld out of range", (long long)B);
    TN_REQUIRE_BUFFER("crl_tron_net_eval");
    CRL_REQUIRE(obs_board && obs_heads && obs_dirs, "crl_tron_net_eval: NULL input pointer");
    CRL_REQUIRE(prior && value, "crl_tron_net_eval: NULL output pointer");
    CRL_REQUIRE(flags == 0, "crl_tron_net_eval: unknown flags 0x%x", flags);
    const tn_layout lay = tn_layout_of(ctx->tron.N, H, L);
    const uint64_t tiles = ((uint64_t)B + 15u) / 16u;
    const unsigned blocks = (unsigned)(tiles < TN_MAX_BLOCKS ? tiles : TN_MAX_BLOCKS);
    switch ((H / 16 + TN_WAVES - 1) / TN_WAVES) {
        TN_EVAL_CASE(1); TN_EVAL_CASE(2); TN_EVAL_CASE(3); TN_EVAL_CASE(4);
    }
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

} // extern "C"
