// ttt_net.hip -- the policy-value MLP between crl_ttt_puct_select and crl_ttt_puct_backup in one launch (crl_ttt_net_*; the
// contract is in include/colosseum_hip.h), gfx950, wave64, float32 MFMA (v_mfma_f32_16x16x4_f32).  DESIGN.md 4.5m states the
// layout below with the measurements.
//
// One wave owns 16 leaves per trip and computes the TRANSPOSED chain Y^T = W X^T: the weight tile is the A operand (16
// outputs x 4 inputs), the activations are the B operand (4 inputs x 16 leaves).  With n = lane % 16 and g = lane / 16 the
// accumulator of output tile T holds, in lane (n, g), outputs 16 T + 4 g + r (r = 0..3) of leaf n.  A B operand wants, in
// lane (n, g), input k = g of leaf n -- so k-step (t, r) of the next layer contracts over feature 16 t + 4 g + r, the very
// value register r of tile t already holds in that lane.  The contraction order is free: the activations never leave their
// registers between layers, no LDS transpose, no cross-lane move.  The matching A fragment of lane (i, g) is
// W[16 T + i][16 t + 4 g .. + 3], one aligned float4 of the row-major matrix, read from the packed buffer through L2 (at
// H = 256 a layer is 256 KB: it does not fit LDS, and at H = 64 every wave reads each weight once per trip anyway).
// The first layer's B operand is the one-hot expansion of the board, built on the fly from the 16 boards of the wave (a
// 16 x cells byte tile in LDS): feature f = cell * C + c is (board[cell] == c), its products are exact.
// The packed network is every matrix padded with zeros to multiples of 16 in both dimensions, each followed by its padded
// bias, in the order hidden layers, policy head, value head: a padded hidden unit is relu(0) = 0 and multiplies zero columns.
// The epilogue stays in registers: the masked maximum of the policy tiles within a lane and across the four lane groups of a
// leaf (two ds_bpermute), exp, scale, round, the sigmoid of the value tile, the stores.
#include "crl_common.hpp"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int NET_MAX_C = 8, NET_MIN_H = 16, NET_MAX_H = 256, NET_MAX_L = 3, NET_MATS = NET_MAX_L + 2;
constexpr int NET_VALUE_ROWS = 16;                               // the value head's P <= 8 rows, padded to one tile
constexpr unsigned NET_MAX_BLOCKS = 2048;                        // one-wave workgroups: two waves a SIMD on 256 CUs, a grid-stride loop past that
static_assert(CRL_TTT_MAX_P <= NET_VALUE_ROWS, "the value head is one tile");

__host__ __device__ inline uint32_t net_pad16(const uint32_t x) { return (x + 15u) & ~15u; }

// where the parts of a packed network lie, in floats (host and device agree on it here and nowhere else)
struct net_layout {
    uint32_t Fp, Np;            // the first layer's padded inputs (cells * C), the policy head's padded rows (cells)
    uint32_t hidden;            // the first of the L - 1 layers H x H, each H * H + H floats
    uint32_t policy, value;     // the heads, each rows * H weights and then rows biases
    uint32_t total;
};

__host__ __device__ inline net_layout net_layout_of(const int cells, const int C, const int H, const int L)
{
    net_layout y;
    const uint32_t h = (uint32_t)H;
    y.Fp = net_pad16((uint32_t)(cells * C));
    y.Np = net_pad16((uint32_t)cells);
    y.hidden = h * y.Fp + h;
    y.policy = y.hidden + (uint32_t)(L - 1) * (h * h + h);
    y.value = y.policy + y.Np * h + y.Np;
    y.total = y.value + (uint32_t)NET_VALUE_ROWS * h + (uint32_t)NET_VALUE_ROWS;     // < 2^18 floats
    return y;
}

// ---- pack: every element of the packed buffer from its place in the caller's matrices, zeros in the padding
struct net_pack_args {
    const float *w[NET_MATS], *b[NET_MATS];
    uint32_t rows[NET_MATS], cols[NET_MATS];     // padded
    uint32_t rrows[NET_MATS], rcols[NET_MATS];   // as the caller holds them ([out, in], row-major)
    int n;
};

__global__ void __launch_bounds__(256)
ttt_net_pack_kernel(const net_pack_args a, float *__restrict__ net, const uint32_t total)
{
    for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < total; e += gridDim.x * 256u) {
        uint32_t at = e;
        float v = 0.0f;
        bool found = false;
#pragma unroll
        for (int s = 0; s < NET_MATS; ++s) {
            if (s < a.n && !found) {
                const uint32_t nw = a.rows[s] * a.cols[s];
                if (at < nw) {
                    const uint32_t r = at / a.cols[s], c = at - r * a.cols[s];
                    if (r < a.rrows[s] && c < a.rcols[s]) v = a.w[s][(size_t)r * a.rcols[s] + c];
                    found = true;
                } else if (at < nw + a.rows[s]) {
                    if (at - nw < a.rrows[s]) v = a.b[s][at - nw];
                    found = true;
                } else {
                    at -= nw + a.rows[s];
                }
            }
        }
        net[e] = v;
    }
}

// ---- eval
__device__ __forceinline__ void net_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ f32x4 net_relu(const f32x4 v)
{
    f32x4 y;
    y.x = fmaxf(v.x, 0.0f), y.y = fmaxf(v.y, 0.0f), y.z = fmaxf(v.z, 0.0f), y.w = fmaxf(v.w, 0.0f);
    return y;
}

// acc += W[16 T + n][16 t + 4 g .. + 3] x (the four inputs this lane holds of input tile t): four k-steps of one MFMA each
__device__ __forceinline__ f32x4 net_mac(const float *__restrict__ w_row, const f32x4 in, f32x4 acc)
{
    const f32x4 a = *reinterpret_cast<const f32x4 *>(w_row);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, in.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, in.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, in.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, in.w, acc, 0, 0, 0);
    return acc;
}

// one head tile: rows 16 T .. 16 T + 15 of a [rows, H] matrix (weights at w, biases at b) over the activations x
template <int HT>
__device__ __forceinline__ f32x4 net_head_tile(const float *__restrict__ w, const float *__restrict__ b, const int T, const int n,
                                               const int g, const f32x4 (&x)[HT])
{
    constexpr int H = 16 * HT;
    f32x4 acc = *reinterpret_cast<const f32x4 *>(b + 16 * T + 4 * g);
    const float *row = w + (size_t)(16 * T + n) * H + 4 * g;
#pragma unroll
    for (int t = 0; t < HT; ++t) acc = net_mac(row + 16 * t, x[t], acc);
    return acc;
}

template <int HT>
__global__ void __launch_bounds__(64)
ttt_net_eval_kernel(const net_layout lay, const int L, const int cells, const int P, const int C, const uint32_t c_magic,
                    const int64_t B, const float *__restrict__ net, const int8_t *__restrict__ board,
                    const uint32_t *__restrict__ valid, const uint8_t *__restrict__ pending, uint16_t *__restrict__ prior,
                    int32_t *__restrict__ value)
{
    constexpr int H = 16 * HT;
    __shared__ int8_t tile[16 * 32];                             // the wave's 16 boards, rows of `cells` bytes
    const int lane = (int)threadIdx.x, n = lane & 15, g = lane >> 4;
    const int64_t tiles = (B + 15) >> 4;
    const int Fp = (int)lay.Fp, n_pol = (int)lay.Np >> 4;        // 1 or 2 policy tiles
    for (int64_t tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
        const int64_t leaf = tl * 16 + n;
        const bool row = leaf < B;
        const bool pend = row && (pending == nullptr || pending[leaf] != 0);
        const int rows_here = (int)min((int64_t)16, B - tl * 16);
        if (__ballot(pend) == 0ull) {                            // nothing to evaluate here: the zeros alone
            for (int i = lane; i < rows_here * cells; i += 64) prior[tl * 16 * cells + i] = 0;
            for (int i = lane; i < rows_here * P; i += 64) value[tl * 16 * P + i] = 0;
            continue;
        }
        net_wave_sync();                                         // the last trip's reads of the tile are over
        for (int i = lane; i < 16 * cells; i += 64) tile[i] = i < rows_here * cells ? board[tl * 16 * cells + i] : (int8_t)-1;
        net_wave_sync();

        // ---- the first layer over the one-hot features, a run-time loop over its k tiles (its B operand is made here)
        f32x4 x[HT], y[HT];
        const float *w0 = net, *b0 = net + (size_t)H * Fp;
#pragma unroll
        for (int T = 0; T < HT; ++T) x[T] = *reinterpret_cast<const f32x4 *>(b0 + 16 * T + 4 * g);
        for (int t = 0; t < Fp; t += 16) {
            f32x4 oh;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint32_t f = (uint32_t)(t + 4 * g + r);    // < 256: (f * ceil(2^16 / C)) >> 16 is f / C for C <= 8
                const uint32_t cell = (f * c_magic) >> 16, c = f - cell * (uint32_t)C;
                const int at = tile[n * cells + (int)min(cell, (uint32_t)cells - 1u)];
                oh[r] = (cell < (uint32_t)cells && at == (int)c) ? 1.0f : 0.0f;
            }
            const float *rowp = w0 + (size_t)n * Fp + t + 4 * g;
#pragma unroll
            for (int T = 0; T < HT; ++T) x[T] = net_mac(rowp + (size_t)(16 * T) * Fp, oh, x[T]);
        }
#pragma unroll
        for (int T = 0; T < HT; ++T) x[T] = net_relu(x[T]);

        // ---- the hidden layers: x -> y in registers, bias and ReLU in place
        for (int l = 1; l < L; ++l) {
            const float *w = net + lay.hidden + (size_t)(l - 1) * (H * H + H), *b = w + H * H;
#pragma unroll
            for (int T = 0; T < HT; ++T) y[T] = *reinterpret_cast<const f32x4 *>(b + 16 * T + 4 * g);
#pragma unroll
            for (int t = 0; t < HT; ++t) {
#pragma unroll
                for (int T = 0; T < HT; ++T) y[T] = net_mac(w + (size_t)(16 * T + n) * H + 16 * t + 4 * g, x[t], y[T]);
            }
#pragma unroll
            for (int T = 0; T < HT; ++T) x[T] = net_relu(y[T]);
        }

        // ---- the heads
        const float *wp = net + lay.policy, *bp = wp + (size_t)lay.Np * H, *wv = net + lay.value, *bv = wv + NET_VALUE_ROWS * H;
        f32x4 pol[2];
        pol[0] = net_head_tile<HT>(wp, bp, 0, n, g, x);
        pol[1] = pol[0];
        if (n_pol > 1) pol[1] = net_head_tile<HT>(wp, bp, 1, n, g, x);
        const f32x4 val = net_head_tile<HT>(wv, bv, 0, n, g, x);

        // ---- the epilogue: the greatest valid logit of the leaf, then exp, scale, round; the sigmoid of the values
        const uint32_t vmask = pend ? valid[leaf] : 0u;
        float top = -INFINITY;
        bool ok[2][4];
#pragma unroll
        for (int T = 0; T < 2; ++T) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int cell = 16 * T + 4 * g + r;             // < 32
                ok[T][r] = T < n_pol && cell < cells && ((vmask >> cell) & 1u);
                top = ok[T][r] ? fmaxf(top, pol[T][r]) : top;
            }
        }
        top = fmaxf(top, __int_as_float(__builtin_amdgcn_ds_bpermute((lane ^ 16) << 2, __float_as_int(top))));
        top = fmaxf(top, __int_as_float(__builtin_amdgcn_ds_bpermute((lane ^ 32) << 2, __float_as_int(top))));
        if (row) {
#pragma unroll
            for (int T = 0; T < 2; ++T) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int cell = 16 * T + 4 * g + r;
                    if (T < n_pol && cell < cells) {
                        const float e = ok[T][r] ? 65535.0f * expf(pol[T][r] - top) : 0.0f;
                        prior[leaf * cells + cell] = (uint16_t)min(max(__float2int_rn(e), 0), 65535);      // (NaN: 0)
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = 4 * g + r;
                if (j < P) {
                    const float s = pend ? 65536.0f / (1.0f + expf(-val[r])) : 0.0f;
                    value[leaf * P + j] = min(max(__float2int_rn(s), 0), 65536);
                }
            }
        }
    }
}

#define NET_REQUIRE_SHAPE(fn)                                                                                                  \
    CRL_REQUIRE(ctx != nullptr && ctx->game == CRL_GAME_TTT, "%s: ctx is not a tictactoe context", fn);                        \
    CRL_REQUIRE(C >= 1 && C <= NET_MAX_C, "%s: C=%d out of range 1..%d", fn, C, NET_MAX_C);                                    \
    CRL_REQUIRE(H >= NET_MIN_H && H <= NET_MAX_H && H % 16 == 0, "%s: H=%d is not a multiple of 16 in %d..%d", fn, H, NET_MIN_H, \
                NET_MAX_H);                                                                                                    \
    CRL_REQUIRE(L >= 1 && L <= NET_MAX_L, "%s: L=%d out of range 1..%d", fn, L, NET_MAX_L)

#define NET_REQUIRE_BUFFER(fn)                                                                                                 \
    CRL_REQUIRE(net != nullptr, "%s: NULL net pointer", fn);                                                                   \
    CRL_REQUIRE((((uintptr_t)net) & 15) == 0, "%s: net must be 16-byte aligned", fn)

} // namespace

extern "C" {

int64_t crl_ttt_net_bytes(const crl_ctx *ctx, int C, int H, int L)
{
    NET_REQUIRE_SHAPE("crl_ttt_net_bytes");
    return (int64_t)net_layout_of(ctx->ttt.n_cells, C, H, L).total * 4;
}

int crl_ttt_net_pack(const crl_ctx *ctx, int C, int H, int L, const float *const *weight, const float *const *bias, void *net,
                     void *stream)
{
    NET_REQUIRE_SHAPE("crl_ttt_net_pack");
    NET_REQUIRE_BUFFER("crl_ttt_net_pack");
    CRL_REQUIRE(weight != nullptr && bias != nullptr, "crl_ttt_net_pack: NULL weight or bias array");
    for (int s = 0; s < L + 2; ++s)
        CRL_REQUIRE(weight[s] != nullptr && bias[s] != nullptr, "crl_ttt_net_pack: NULL weight or bias pointer of matrix %d", s);
    const int cells = ctx->ttt.n_cells;
    const net_layout lay = net_layout_of(cells, C, H, L);
    net_pack_args a = {};
    a.n = L + 2;
    for (int s = 0; s < a.n; ++s) {
        a.w[s] = weight[s], a.b[s] = bias[s];
        const bool pol = s == L, val = s == L + 1;
        a.rrows[s] = (uint32_t)(pol ? cells : (val ? ctx->ttt.P : H));
        a.rows[s] = pol ? lay.Np : (val ? (uint32_t)NET_VALUE_ROWS : (uint32_t)H);
        a.rcols[s] = (uint32_t)(s == 0 ? cells * C : H);
        a.cols[s] = s == 0 ? lay.Fp : (uint32_t)H;
    }
    hipLaunchKernelGGL(ttt_net_pack_kernel, dim3((lay.total + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, a,
                       static_cast<float *>(net), lay.total);
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

#define NET_EVAL_CASE(HT_)                                                                                                     \
    case HT_:                                                                                                                  \
        hipLaunchKernelGGL(ttt_net_eval_kernel<HT_>, dim3(blocks), dim3(64), 0, (hipStream_t)stream, lay, L, cells, ctx->ttt.P, C, \
                           c_magic, B, static_cast<const float *>(net), board, valid, pending, prior, value);                  \
        break

int crl_ttt_net_eval(const crl_ctx *ctx, int64_t B, const void *net, int C, int H, int L, const int8_t *board, const uint32_t *valid,
                     const uint8_t *pending, uint16_t *prior, int32_t *value, uint32_t flags, void *stream)
{
    NET_REQUIRE_SHAPE("crl_ttt_net_eval");
    CRL_REQUIRE(B > 0 && B <= ((int64_t)1 << 31), "crl_ttt_net_eval: B=%lld out of range", (long long)B);
    NET_REQUIRE_BUFFER("crl_ttt_net_eval");
    CRL_REQUIRE(board && valid, "crl_ttt_net_eval: NULL input pointer");
    CRL_REQUIRE(prior && value, "crl_ttt_net_eval: NULL output pointer");
    CRL_REQUIRE(flags == 0, "crl_ttt_net_eval: unknown flags 0x%x", flags);
    const int cells = ctx->ttt.n_cells;
    const net_layout lay = net_layout_of(cells, C, H, L);
    const uint32_t c_magic = (65536u + (uint32_t)C - 1u) / (uint32_t)C;
    const uint64_t tiles = ((uint64_t)B + 15u) / 16u;
    const unsigned blocks = (unsigned)(tiles < NET_MAX_BLOCKS ? tiles : NET_MAX_BLOCKS);
    switch (H / 16) {
        NET_EVAL_CASE(1); NET_EVAL_CASE(2); NET_EVAL_CASE(3); NET_EVAL_CASE(4); NET_EVAL_CASE(5); NET_EVAL_CASE(6);
        NET_EVAL_CASE(7); NET_EVAL_CASE(8); NET_EVAL_CASE(9); NET_EVAL_CASE(10); NET_EVAL_CASE(11); NET_EVAL_CASE(12);
        NET_EVAL_CASE(13); NET_EVAL_CASE(14); NET_EVAL_CASE(15); NET_EVAL_CASE(16);
    }
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

} // extern "C"
