// ttt_puct_search.hip -- the whole network-valued TicTacToe search in ONE launch (crl_ttt_puct_search; the contract is in
// include/colosseum_hip.h), gfx950, wave64.  It leaves in the trees what n_sims repetitions of crl_ttt_puct_select,
// crl_ttt_net_eval and crl_ttt_puct_backup leave, byte for byte: the descent and the backup are ttt_puct.hip's, the MLP is
// ttt_net.hip's arithmetic in ttt_net.hip's order, restated here so that those kernels stay what they are.  DESIGN.md 4.5n
// holds the layout, the LDS map and the measurements.
//
// A workgroup of 8 waves owns 16 trees -- one MFMA tile of leaves -- for all n_sims simulations; wave i owns trees 2 i and
// 2 i + 1 in every phase, so a tree's nodes are read and written by one wave only and HBM needs no ordering between waves
// (16 waves of one tree would be capped at 128 VGPRs, which the 13-direction descent does not fit).  A simulation is
//   1  descent (select's, lanes = cells); the leaf goes, as its mover sees it, into a 16 x 32 byte tile in LDS, its pending
//      flag beside it; the path, the empties mask and the movers stay in the wave's registers           -> workgroup barrier
//   2  the MLP, dealt over the waves by OUTPUT tile (a run-time loop: no template over the width); every sum keeps
//      crl_ttt_net_eval's order: the bias first, k-steps (t, r) ascending.  Activations pass from layer to layer through two
//      LDS buffers, a barrier per layer; the heads leave 32 logits and 16 values per leaf in LDS.  Skipped when no leaf of the
//      16 is pending
//   3  epilogue and backup by the owning wave, lanes = cells: masked maximum, exp / scale / round, backup's normalisation,
//      the n / w update along the path held in registers.  Priors and values never reach HBM             -> wave fence
// Unlike select and backup, the lanes of a wave here read through memory what other lanes wrote earlier in the launch
// (child slots, n / w, priors): the wave fence after phase 3 orders that.
// The packed network is copied into LDS once per launch when it fits beside the rest (PS_LDS_BUDGET), rows padded by four
// floats so that the 16 rows of an A fragment fall on different banks; wider networks are read through L2 as
// ttt_net_eval_kernel reads them.
#define TTT_DEVICE_ONLY
#include "ttt.hip"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- the tree (ttt_puct.hip states the layout)
constexpr int PUCT_H_NODES = 0, PUCT_H_SIMS = 1, PUCT_H_LEAF = 3, PUCT_H_MOVER0 = 4, PUCT_H_LEAF_E = 5,
              PUCT_H_LEAF_MOVER = 6, PUCT_H_OCC = 8;
constexpr int PUCT_HDR_BYTES = 64, PUCT_PATH_SLOTS = 40, PUCT_FIXED_BYTES = PUCT_HDR_BYTES + 2 * PUCT_PATH_SLOTS;
constexpr uint32_t PUCT_PENDING = 1u, PUCT_TERMINAL = 2u;
constexpr int PUCT_MAX_S = 4095;

__host__ __device__ inline uint64_t puct_tree_bytes(const int S_cap, const int cells)
{
    const uint64_t N = (uint64_t)S_cap + 1u;
    return ((uint64_t)PUCT_FIXED_BYTES + N * (8u + 4u * (uint64_t)cells) + 15u) & ~(uint64_t)15u;
}

struct puct_tree {
    uint32_t *hdr;
    uint16_t *path;
    uint32_t *n, *w;
    uint16_t *prior, *child;
};

__device__ __forceinline__ puct_tree puct_tree_of(uint8_t *trees, const int64_t b, const uint64_t tree_bytes, const int S_cap, const int cells)
{
    uint8_t *base = trees + (uint64_t)b * tree_bytes;
    const uint32_t N = (uint32_t)S_cap + 1u;
    puct_tree t;
    t.hdr = reinterpret_cast<uint32_t *>(base);
    t.path = reinterpret_cast<uint16_t *>(base + PUCT_HDR_BYTES);
    t.n = reinterpret_cast<uint32_t *>(base + PUCT_FIXED_BYTES);
    t.w = t.n + N;
    t.prior = reinterpret_cast<uint16_t *>(t.w + N);
    t.child = t.prior + (size_t)N * (size_t)cells;
    return t;
}

// the maximum / the sum of v over the 64 lanes, in every lane; a lane without a source sees 0 (every lane must run them)
__device__ __forceinline__ uint32_t puct_wave_max(uint32_t v)
{
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false));   // row_shr:1
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false));   // row_shr:2
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false));   // row_shr:4
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false));   // row_shr:8
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));   // row_bcast:15 -> rows 1, 3
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));   // row_bcast:31 -> rows 2, 3
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

__device__ __forceinline__ uint32_t puct_wave_sum(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// the same steps over floats, -inf where a lane has no source (the maximum does not depend on the order it is taken in)
__device__ __forceinline__ float ps_wave_fmax(float v)
{
    const int none = __float_as_int(-INFINITY);
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(none, __float_as_int(v), 0x111, 0xf, 0xf, false)));
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(none, __float_as_int(v), 0x112, 0xf, 0xf, false)));
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(none, __float_as_int(v), 0x114, 0xf, 0xf, false)));
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(none, __float_as_int(v), 0x118, 0xf, 0xf, false)));
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(none, __float_as_int(v), 0x142, 0xa, 0xf, false)));
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(none, __float_as_int(v), 0x143, 0xc, 0xf, false)));
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

__device__ __forceinline__ uint64_t puct_div(const uint64_t num, const uint32_t den)
{
    uint64_t q = (uint64_t)((double)num / (double)den);
    const int64_t r = (int64_t)(num - q * (uint64_t)den);
    q = r < 0 ? q - 1u : (r >= (int64_t)den ? q + 1u : q);
    return q;
}

__device__ __forceinline__ uint64_t puct_isqrt(const uint64_t x)
{
    uint64_t s = (uint64_t)sqrt((double)x);
    s = s * s > x ? s - 1u : ((s + 1u) * (s + 1u) <= x ? s + 1u : s);
    return s;
}

__device__ __forceinline__ uint32_t puct_in_vgpr(const uint32_t x)
{
    uint32_t v;
    asm("v_mov_b32 %0, %1" : "=v"(v) : "s"(x));
    return v;
}

// ---- the packed network (ttt_net.hip states the layout)
constexpr int NET_MAX_C = 8, NET_MIN_H = 16, NET_MAX_H = 256, NET_MAX_L = 3, NET_MATS = NET_MAX_L + 2;
constexpr int NET_VALUE_ROWS = 16;

__host__ __device__ inline uint32_t net_pad16(const uint32_t x) { return (x + 15u) & ~15u; }

// ---- this kernel's geometry
constexpr int PS_TREES = 16, PS_WAVES = 8, PS_TPW = PS_TREES / PS_WAVES, PS_THREADS = 64 * PS_WAVES;   // two trees a wave: DESIGN.md 4.5n has the reason
constexpr unsigned PS_MAX_BLOCKS = 512;                          // two workgroups a CU on 256 CUs, a grid-stride loop past that
constexpr int PS_PAD = 4;                                        // floats added to a row of weights or activations in LDS
constexpr uint32_t PS_LDS_BUDGET = 160u * 1024u;                 // all of a CU's LDS: the weights go there when everything fits
static_assert(PS_TREES == PS_WAVES * PS_TPW, "wave i owns trees PS_TPW i .. PS_TPW i + PS_TPW - 1");

// where the matrices of the packed network lie, in floats: in the packed buffer and, when they are staged, in LDS
struct ps_net {
    uint32_t src[NET_MATS], dst[NET_MATS], rows[NET_MATS], cols[NET_MATS];   // hidden layers, policy head, value head
    int n_mats, H, L, n_pol, in_lds;
    uint32_t lds_bytes;
};

// the LDS map in floats: two activation buffers, the logits, the values, the board tile, two sets of pending flags, weights
__host__ __device__ inline uint32_t ps_act_stride(const int H) { return (uint32_t)(H + PS_PAD); }
constexpr uint32_t PS_LOGIT_FLOATS = PS_TREES * 32, PS_VALUE_FLOATS = PS_TREES * NET_VALUE_ROWS, PS_TILE_FLOATS = PS_TREES * 32 / 4,
                   PS_FLAG_FLOATS = 2 * PS_TREES / 4;
__host__ __device__ inline uint32_t ps_fixed_floats(const int H)
{
    return 2u * PS_TREES * ps_act_stride(H) + PS_LOGIT_FLOATS + PS_VALUE_FLOATS + PS_TILE_FLOATS + PS_FLAG_FLOATS;
}

inline ps_net ps_net_of(const int cells, const int C, const int H, const int L)
{
    ps_net y = {};
    y.n_mats = L + 2, y.H = H, y.L = L;
    const uint32_t Np = net_pad16((uint32_t)cells);
    y.n_pol = (int)(Np >> 4);
    uint32_t src = 0, dst = 0;
    for (int s = 0; s < y.n_mats; ++s) {
        y.rows[s] = s == L ? Np : (s == L + 1 ? (uint32_t)NET_VALUE_ROWS : (uint32_t)H);
        y.cols[s] = s == 0 ? net_pad16((uint32_t)(cells * C)) : (uint32_t)H;
        y.src[s] = src, y.dst[s] = dst;
        src += y.rows[s] * y.cols[s] + y.rows[s];
        dst += y.rows[s] * (y.cols[s] + PS_PAD) + y.rows[s];
    }
    const uint32_t fixed = ps_fixed_floats(H) * 4u;
    y.in_lds = fixed + dst * 4u <= PS_LDS_BUDGET;
    y.lds_bytes = fixed + (y.in_lds ? dst * 4u : 0u);
    return y;
}

__device__ __forceinline__ void ps_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// acc += the four k-steps (t, 0..3) of one output tile: the A fragment a float4 of the weight row, the B operands in `in`
__device__ __forceinline__ f32x4 ps_mac(const f32x4 a, const f32x4 in, f32x4 acc)
{
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, in.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, in.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, in.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, in.w, acc, 0, 0, 0);
    return acc;
}

// where matrix s is read from: LDS (rows padded) or the packed buffer
template <bool WL>
struct ps_mat {
    const float *w, *b;
    uint32_t stride;
    __device__ __forceinline__ ps_mat(const ps_net &pn, const int s, const float *net, const float *wl)
    {
        stride = pn.cols[s] + (WL ? (uint32_t)PS_PAD : 0u);
        w = (WL ? wl + pn.dst[s] : net + pn.src[s]);
        b = w + pn.rows[s] * stride;
    }
};

// output tile T of a layer over the activations in `x` (16 leaves, stride xs): the bias, then k tiles 0 .. kt - 1 in order
template <bool WL>
__device__ __forceinline__ f32x4 ps_tile(const ps_mat<WL> &m, const int T, const int kt, const float *x, const uint32_t xs, const int n,
                                         const int g)
{
    f32x4 acc = *reinterpret_cast<const f32x4 *>(m.b + 16 * T + 4 * g);
    const float *row = m.w + (size_t)(16 * T + n) * m.stride + 4 * g;
    const float *in = x + (size_t)n * xs + 4 * g;
    for (int t = 0; t < kt; ++t)
        acc = ps_mac(*reinterpret_cast<const f32x4 *>(row + 16 * t), *reinterpret_cast<const f32x4 *>(in + 16 * t), acc);
    return acc;
}

__device__ __forceinline__ f32x4 ps_relu(const f32x4 v)
{
    f32x4 y;
    y.x = fmaxf(v.x, 0.0f), y.y = fmaxf(v.y, 0.0f), y.z = fmaxf(v.z, 0.0f), y.w = fmaxf(v.w, 0.0f);
    return y;
}

// ---- phase 2: the 16 leaves of the board tile through the network; logits and values of every leaf into LDS.  The whole
// workgroup runs it (it holds barriers); wave `wave` computes output tiles wave, wave + PS_WAVES, ... of every layer.
template <bool WL>
__device__ __forceinline__ void ps_mlp(const ps_net &pn, const float *net, const float *wl, const int cells, const int C,
                                       const uint32_t c_magic, const int8_t *tile, float *act0, float *act1, float *logit, float *valf,
                                       const int wave, const int lane)
{
    const int n = lane & 15, g = lane >> 4, HT = pn.H >> 4;
    const uint32_t xs = ps_act_stride(pn.H);
    {   // the first layer: its B operand is the one-hot expansion of the board, made here
        const ps_mat<WL> m(pn, 0, net, wl);
        const int kt = (int)pn.cols[0] >> 4;
        for (int T = wave; T < HT; T += PS_WAVES) {
            f32x4 acc = *reinterpret_cast<const f32x4 *>(m.b + 16 * T + 4 * g);
            const float *row = m.w + (size_t)(16 * T + n) * m.stride + 4 * g;
            for (int t = 0; t < kt; ++t) {
                f32x4 oh;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const uint32_t f = (uint32_t)(16 * t + 4 * g + r);   // < 256: (f * ceil(2^16 / C)) >> 16 is f / C for C <= 8
                    const uint32_t cell = (f * c_magic) >> 16, c = f - cell * (uint32_t)C;
                    const int at = tile[n * 32 + (int)min(cell, (uint32_t)cells - 1u)];
                    oh[r] = (cell < (uint32_t)cells && at == (int)c) ? 1.0f : 0.0f;
                }
                acc = ps_mac(*reinterpret_cast<const f32x4 *>(row + 16 * t), oh, acc);
            }
            *reinterpret_cast<f32x4 *>(act0 + (size_t)n * xs + 16 * T + 4 * g) = ps_relu(acc);
        }
        __syncthreads();
    }
    float *x = act0, *y = act1;
    for (int l = 1; l < pn.L; ++l) {
        const ps_mat<WL> m(pn, l, net, wl);
        for (int T = wave; T < HT; T += PS_WAVES)
            *reinterpret_cast<f32x4 *>(y + (size_t)n * xs + 16 * T + 4 * g) = ps_relu(ps_tile<WL>(m, T, HT, x, xs, n, g));
        __syncthreads();
        float *swap = x;
        x = y, y = swap;
    }
    // the heads: the policy tiles, then the value tile
    for (int T = wave; T <= pn.n_pol; T += PS_WAVES) {
        if (T < pn.n_pol) {
            const ps_mat<WL> m(pn, pn.L, net, wl);
            *reinterpret_cast<f32x4 *>(logit + n * 32 + 16 * T + 4 * g) = ps_tile<WL>(m, T, HT, x, xs, n, g);
        } else {
            const ps_mat<WL> m(pn, pn.L + 1, net, wl);
            *reinterpret_cast<f32x4 *>(valf + n * NET_VALUE_ROWS + 4 * g) = ps_tile<WL>(m, 0, HT, x, xs, n, g);
        }
    }
    __syncthreads();
}

// what a wave keeps of its tree between the descent and the backup of a simulation
struct ps_leaf {
    uint32_t path;              // lane i: the node at depth i
    uint32_t E;                 // the leaf's empties mask
    int tm0, tm, d, ws;         // the root's mover, the leaf's mover, the leaf's depth, the winner of a terminal leaf
    bool pend, have;
};

// ---- phase 1: select's descent of one tree (ttt_puct_select_kernel, statement for statement), the leaf's row of the board
// tile and its pending flag.  The header is written once a simulation, by ps_backup.
template <int P, int ND>
__device__ __forceinline__ ps_leaf ps_descend(const ttt_dirs &dd, const puct_tree &t, const bool live, const int S_cap, const uint32_t cpuct,
                                              const uint32_t fpu, const int rel_mod, const int lane, uint32_t &nn, const uint32_t sims,
                                              int8_t *tile_row, uint8_t *flag)
{
    const int cells = dd.n_cells;
    uint32_t o[P];
#pragma unroll
    for (int p = 0; p < P; ++p) o[p] = 0u;
    ps_leaf lf;
    lf.path = 0, lf.E = 0, lf.tm0 = 0, lf.tm = -1, lf.d = 0, lf.ws = -1, lf.pend = false, lf.have = false;
    if (live) {
        bool descend = sims < (uint32_t)S_cap;
        int w = -1, v = 0, d = 0, term = 0, ws = -1, rw, tm = -1;
        uint32_t path = 0;
        bool pend = false;
        if (descend) {
#pragma unroll
            for (int p = 0; p < P; ++p) o[p] = t.hdr[PUCT_H_OCC + p];
            tm = (int)t.hdr[PUCT_H_MOVER0];
            lf.tm0 = tm;
        }
        while (descend) {
            CRL_BOUNDS_LT(v, S_cap + 1, 240);
            const uint32_t nv = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.n[v]);
            if (nv == 0u) { pend = true; break; }               // an unexpanded node: the pending leaf
            const uint32_t E = dd.full & ~ttt_union<P>(o);
            const bool in_e = lane < 32 && ((E >> (lane & 31)) & 1u);
            const size_t at = (size_t)v * (size_t)cells + (size_t)lane;
            const uint32_t pe = in_e ? t.prior[at] : 0u;
            uint32_t cu = in_e ? t.child[at] : 0u;
            CRL_BOUNDS_LT(cu, S_cap + 1, 241);
            cu = min(cu, (uint32_t)S_cap);
            const uint64_t rt = puct_isqrt((uint64_t)nv << 16);
            uint32_t key = 0;
            if (in_e) {
                const uint32_t nu = cu ? t.n[cu] : 0u, wu = cu ? t.w[cu] : 0u;
                const uint64_t exploit = nu ? puct_div(wu, nu) : (uint64_t)fpu;
                const uint64_t explore = puct_div((uint64_t)cpuct * pe * rt, (1u + min(nu, 4095u)) << 16);
                key = (uint32_t)(exploit + explore) + 1u;
            }
            const uint32_t top = puct_wave_max(key);             // (all lanes: outside the branch above)
            const unsigned long long at_top = __ballot(in_e && key == top);
            if (at_top == 0ull) break;                           // (never: a running position has an empty cell)
            const int e = (int)__builtin_ctzll(at_top);          // ties: the lowest cell
            int u = __builtin_amdgcn_readlane((int)cu, e);
            const bool fresh = u == 0;
            if (fresh) {
                if (nn > (uint32_t)S_cap) break;                 // (never: nodes <= simulations + 2 <= S_cap + 1)
                u = (int)nn++;
                CRL_BOUNDS_LT(u, S_cap + 1, 242);
                if (lane == e) t.child[at] = (uint16_t)u;
                if (lane < cells) {
                    t.prior[(size_t)u * (size_t)cells + (size_t)lane] = 0;
                    t.child[(size_t)u * (size_t)cells + (size_t)lane] = 0;
                }
                if (lane == 0) { t.n[u] = 0u; t.w[u] = 0u; }
            }
            d += 1;
            path = lane == d ? (uint32_t)u : path;
            ttt_step_core<P, ND>(dd, o, w, tm, e, rw, term, ws);
            term = __builtin_amdgcn_readfirstlane(term);         // (every lane played the same ply)
            ws = __builtin_amdgcn_readfirstlane(ws);
            if (term) break;
            if (fresh) { pend = true; break; }                   // the new node is the leaf: nothing of it is read in this descent
            if (d >= 32) break;                                  // (never: a ply that fills the board is terminal)
            v = u;
        }
        lf.have = pend || term;
        CRL_BOUNDS_LT(d, PUCT_PATH_SLOTS, 243);
        if (lf.have && lane <= d) t.path[lane] = (uint16_t)path;
        lf.path = path, lf.E = dd.full & ~ttt_union<P>(o), lf.tm = tm, lf.d = d, lf.ws = ws, lf.pend = pend;
    }
    // the pending leaf as its mover sees it (select's rule, lane = cell); every other row of the tile is an empty board
    if (lane < 32) {
        int c = -1;
        if (lf.pend) {
#pragma unroll
            for (int p = 0; p < P; ++p) c = ((o[p] >> (lane & 31)) & 1u) ? p : c;
            if (c >= 0) {
                const int rr = (c - lf.tm) % rel_mod;
                c = rr < 0 ? rr + rel_mod : rr;
            }
        }
        tile_row[lane] = (int8_t)c;
    }
    if (lane == 0) *flag = lf.pend ? 1 : 0;
    return lf;
}

// ---- phase 3: crl_ttt_net_eval's epilogue and ttt_puct_backup_kernel for one tree, then the header words select and backup
// leave behind (lane i writes word i; the path length is 0 again once the backup has run)
template <int P>
__device__ __forceinline__ void ps_backup(const puct_tree &t, const ps_leaf &lf, const int cells, const int S_cap, const int lane,
                                          const uint32_t nn, uint32_t &sims, const float *logit_row, const float *value_row)
{
    const int plen = lf.d + 1;
    if (lf.have) {
        if (lf.pend) {
            const bool in_e = lane < 32 && ((lf.E >> (lane & 31)) & 1u);
            const float l = logit_row[lane & 31];
            const float top = ps_wave_fmax(in_e ? l : -INFINITY);                 // (all lanes)
            const float e = in_e ? 65535.0f * expf(l - top) : 0.0f;
            const uint32_t pr = in_e ? (uint32_t)min(max(__float2int_rn(e), 0), 65535) : 0u;   // (NaN: 0)
            const uint32_t leaf = min((uint32_t)__builtin_amdgcn_readlane((int)lf.path, lf.d), (uint32_t)S_cap);
            CRL_BOUNDS_LT(__builtin_amdgcn_readlane((int)lf.path, lf.d), S_cap + 1, 244);
            const uint32_t sum = puct_wave_sum(pr);              // (all lanes) <= 32 * 65535
            const uint32_t n_e = max((uint32_t)__popc(lf.E), 1u);
            uint32_t slot = 0;
            if (in_e) slot = (uint32_t)min((uint64_t)65535u, sum ? puct_div((uint64_t)pr << 16, sum) : puct_div(65536u, n_e));
            if (lane < cells) t.prior[(size_t)leaf * (size_t)cells + (size_t)lane] = (uint16_t)slot;
        }
        if (lane < plen) {
            CRL_BOUNDS_LT(lf.path, S_cap + 1, 245);
            const uint32_t node = min(lf.path, (uint32_t)S_cap);
            uint32_t add = 0;
            if (lane > 0) {
                const int q = (lf.tm0 + lane - 1) % P;           // who moved into the node at depth `lane`
                if (lf.pend) {
                    const int j = (q - lf.tm + P) % P;
                    CRL_BOUNDS_LT(j, P, 246);
                    const float s = 65536.0f / (1.0f + expf(-value_row[j]));
                    add = (uint32_t)min(max(__float2int_rn(s), 0), 65536);
                } else {
                    add = lf.ws < 0 ? 32768u : (lf.ws == q ? 65536u : 0u);
                }
            }
            t.n[node] += 1u;
            t.w[node] += add;
        }
        sims += 1u;
    }
    uint32_t word = 0;
    word = lane == PUCT_H_NODES ? nn : word;
    word = lane == PUCT_H_SIMS ? sims : word;
    word = lane == PUCT_H_LEAF ? ((lf.pend ? PUCT_PENDING : PUCT_TERMINAL) | ((uint32_t)(lf.ws + 1) << 8)) : word;
    word = lane == PUCT_H_LEAF_E ? lf.E : word;
    word = lane == PUCT_H_LEAF_MOVER ? (uint32_t)lf.tm : word;
    if (lane < 7 && lane != PUCT_H_MOVER0) t.hdr[lane] = word;   // (word 2, the path length, is 0)
}

template <int P, int ND>
__global__ void __launch_bounds__(PS_THREADS)
ttt_puct_search_kernel(const ttt_dirs dd_arg, const int64_t B, uint8_t *trees, const uint64_t tree_bytes, const int S_cap,
                       const int n_sims, const uint32_t cpuct, const uint32_t fpu, const int rel_mod, const float *__restrict__ net,
                       const ps_net pn, const int C, const uint32_t c_magic)
{
    extern __shared__ __attribute__((aligned(16))) float ps_lds[];
    const uint32_t xs = ps_act_stride(pn.H);
    float *act0 = ps_lds, *act1 = act0 + PS_TREES * xs, *logit = act1 + PS_TREES * xs, *valf = logit + PS_LOGIT_FLOATS;
    int8_t *tile = reinterpret_cast<int8_t *>(valf + PS_VALUE_FLOATS);
    uint8_t *flags = reinterpret_cast<uint8_t *>(tile + PS_TREES * 32);
    float *wl = ps_lds + ps_fixed_floats(pn.H);

    ttt_dirs dd = dd_arg;                                        // (as ttt_puct_select_kernel: the scalar registers do not hold them)
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        dd.stride[d] = (int32_t)puct_in_vgpr((uint32_t)dd_arg.stride[d]);
        dd.start[d] = puct_in_vgpr(dd_arg.start[d]);
    }
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const int cells = dd.n_cells;

    if (pn.in_lds) {                                             // the packed network into LDS, once: rows re-strided, biases behind
        for (int s = 0; s < pn.n_mats; ++s) {
            const uint32_t c4 = pn.cols[s] >> 2, n4 = pn.rows[s] * c4, stride = pn.cols[s] + PS_PAD;
            for (uint32_t i = threadIdx.x; i < n4; i += PS_THREADS) {
                const uint32_t r = i / c4, c = i - r * c4;
                *reinterpret_cast<f32x4 *>(wl + pn.dst[s] + r * stride + 4u * c) =
                    *reinterpret_cast<const f32x4 *>(net + pn.src[s] + r * pn.cols[s] + 4u * c);
            }
            for (uint32_t i = threadIdx.x; i < pn.rows[s] >> 2; i += PS_THREADS)
                *reinterpret_cast<f32x4 *>(wl + pn.dst[s] + pn.rows[s] * stride + 4u * i) =
                    *reinterpret_cast<const f32x4 *>(net + pn.src[s] + pn.rows[s] * pn.cols[s] + 4u * i);
        }
        __syncthreads();
    }

    const int64_t groups = (B + PS_TREES - 1) / PS_TREES;
    uint32_t trip = 0;                                           // the flags alternate between two sets: a wave may be a phase ahead
    for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        int64_t tb[PS_TPW];                                       // this wave's trees; a missing row of a ragged group: an empty board, no tree
        uint32_t nn[PS_TPW], sims[PS_TPW];
        bool live[PS_TPW];
#pragma unroll
        for (int k = 0; k < PS_TPW; ++k) {
            const int64_t b = grp * PS_TREES + wave * PS_TPW + k;
            const bool row = b < B;
            tb[k] = row ? b : 0;
            const puct_tree t = puct_tree_of(trees, tb[k], tree_bytes, S_cap, cells);
            nn[k] = row ? (uint32_t)__builtin_amdgcn_readfirstlane((int)t.hdr[PUCT_H_NODES]) : 0u;
            sims[k] = row ? (uint32_t)__builtin_amdgcn_readfirstlane((int)t.hdr[PUCT_H_SIMS]) : 0u;
            live[k] = nn[k] != 0u && nn[k] <= (uint32_t)S_cap + 1u;              // (a skipped tree is left alone)
        }
        for (int s = 0; s < n_sims; ++s, ++trip) {
            uint8_t *flag = flags + PS_TREES * (trip & 1u);
            ps_leaf lf[PS_TPW];
#pragma unroll
            for (int k = 0; k < PS_TPW; ++k) {
                const int slot = wave * PS_TPW + k;
                lf[k] = ps_descend<P, ND>(dd, puct_tree_of(trees, tb[k], tree_bytes, S_cap, cells), live[k], S_cap, cpuct, fpu, rel_mod,
                                          lane, nn[k], sims[k], tile + slot * 32, flag + slot);
            }
            __syncthreads();
            if (__ballot(lane < PS_TREES && flag[lane & (PS_TREES - 1)] != 0) != 0ull) {   // (alike in every wave)
                if (pn.in_lds) ps_mlp<true>(pn, net, wl, cells, C, c_magic, tile, act0, act1, logit, valf, wave, lane);
                else ps_mlp<false>(pn, net, wl, cells, C, c_magic, tile, act0, act1, logit, valf, wave, lane);
            }
#pragma unroll
            for (int k = 0; k < PS_TPW; ++k) {
                const int slot = wave * PS_TPW + k;
                if (live[k])
                    ps_backup<P>(puct_tree_of(trees, tb[k], tree_bytes, S_cap, cells), lf[k], cells, S_cap, lane, nn[k], sims[k],
                                 logit + slot * 32, valf + slot * NET_VALUE_ROWS);
            }
            ps_wave_sync();                                      // the next descent reads what these lanes stored
        }
    }
}

} // namespace

int crl_ttt_puct_search_bounds(unsigned int *out4)
{
    CRL_BOUNDS_READBACK(out4);
    return CRL_OK;
}

extern "C" {

int crl_ttt_puct_search(const crl_ctx *ctx, int64_t B, void *tree, int S_cap, int n_sims, const void *net, int C, int H, int L,
                        uint32_t cpuct, uint32_t fpu, int rel_mod, uint32_t flags, void *stream)
{
    const char *fn = "crl_ttt_puct_search";
    TTT_CTX_CHECK(fn);
    CRL_REQUIRE(tree != nullptr, "%s: NULL tree pointer", fn);
    CRL_REQUIRE((((uintptr_t)tree) & 15) == 0, "%s: tree must be 16-byte aligned", fn);
    CRL_REQUIRE(S_cap >= 1 && S_cap <= PUCT_MAX_S, "%s: S_cap=%d out of range 1..%d", fn, S_cap, PUCT_MAX_S);
    CRL_REQUIRE(ctx->ttt.n_cells >= ctx->ttt.P, "%s: a board of %d cells for %d players (as crl_ttt_playout)", fn, ctx->ttt.n_cells,
                ctx->ttt.P);
    CRL_REQUIRE(n_sims >= 1 && n_sims <= PUCT_MAX_S, "%s: n_sims=%d out of range 1..%d", fn, n_sims, PUCT_MAX_S);
    CRL_REQUIRE(C >= 1 && C <= NET_MAX_C, "%s: C=%d out of range 1..%d", fn, C, NET_MAX_C);
    CRL_REQUIRE(H >= NET_MIN_H && H <= NET_MAX_H && H % 16 == 0, "%s: H=%d is not a multiple of 16 in %d..%d", fn, H, NET_MIN_H,
                NET_MAX_H);
    CRL_REQUIRE(L >= 1 && L <= NET_MAX_L, "%s: L=%d out of range 1..%d", fn, L, NET_MAX_L);
    CRL_REQUIRE(net != nullptr, "%s: NULL net pointer", fn);
    CRL_REQUIRE((((uintptr_t)net) & 15) == 0, "%s: net must be 16-byte aligned", fn);
    CRL_REQUIRE(cpuct <= 65535u, "%s: cpuct=%u out of range 0..65535", fn, cpuct);
    CRL_REQUIRE(fpu <= 65536u, "%s: fpu=%u out of range 0..65536", fn, fpu);
    CRL_REQUIRE(rel_mod >= 1, "%s: rel_mod must be >= 1 (as crl_ttt_board with a player)", fn);
    CRL_REQUIRE(flags == 0, "%s: unknown flags 0x%x", fn, flags);
    const int cells = ctx->ttt.n_cells;
    const uint64_t tree_bytes = puct_tree_bytes(S_cap, cells);
    const ps_net pn = ps_net_of(cells, C, H, L);
    const uint32_t c_magic = (65536u + (uint32_t)C - 1u) / (uint32_t)C;
    const uint64_t groups = ((uint64_t)B + PS_TREES - 1u) / PS_TREES;
    const unsigned blocks = (unsigned)(groups < PS_MAX_BLOCKS ? groups : PS_MAX_BLOCKS);
    const ttt_dirs dd = ctx->ttt_dd;
    TTT_DISPATCH_ND(ctx, {
        const auto kernel = ttt_puct_search_kernel<PP, NDD>;
        if (pn.lds_bytes > 64u * 1024u)                          // (more than 64 KB of dynamic LDS is an opt-in)
            CRL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)pn.lds_bytes));
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(PS_THREADS), pn.lds_bytes, (hipStream_t)stream, dd, B,
                           static_cast<uint8_t *>(tree), tree_bytes, S_cap, n_sims, cpuct, fpu, rel_mod, static_cast<const float *>(net),
                           pn, C, c_magic);
    });
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

} // extern "C"
