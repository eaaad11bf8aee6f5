// ttt_puct.hip -- tree search valued by the caller's network for TicTacToe (crl_ttt_puct_*; the contract is in
// include/colosseum_hip.h), gfx950, wave64.  The ply, the direction tables and the dispatch macros are ttt.hip's, taken in by
// including that file up to its kernels; the search is a translation unit of its own so that those kernels stay what they
// are (DESIGN.md 4.5j holds the comparison).
//
// The trees live in the caller's buffer in HBM between the launches, one wave per tree in every kernel.  A tree of
// N = S_cap + 1 nodes is, in bytes:
//   [0, 64)      16 header words: node count (0 = a skipped tree), simulation count, path length (0 = no path outstanding),
//                leaf word (kind | (winner + 1) << 8), the root's mover, the leaf's empties mask, the leaf's mover, one
//                spare word, the root's P occupancy words (8 slots)
//   [64, 144)    the path, uint16 [40]: the node at each depth (at most cells + 1 = 33 are used)
//   then         n uint32 [N], w uint32 [N], prior uint16 [N][cells], child uint16 [N][cells] (0 = none)
// rounded up to 16 bytes.  A node's priors and child slots are contiguous, so a level of the descent is one load of each by
// the lanes of the cells, and each lane gathers n and w of its own child.
// "Expanded" has no bit of its own: a descent only ever stands on the root or on a node it reached by a ply that did not end
// the game, and such a node has priors exactly when a backup has passed through it, which is n > 0 (a fresh node has n = 0
// until the backup of the simulation that made it, and that backup gives it its priors).
// No lane reads through memory what another lane of the same launch wrote: a fresh node is the leaf (nothing of it is read
// back), the path is written at the end of select and read by backup, a launch later.  So the kernels carry no wave fences.
// Every index read out of the tree is clamped to S_cap before it addresses anything: a buffer that was never given to
// crl_ttt_puct_begin cannot make a kernel write outside it.
#define TTT_DEVICE_ONLY
#include "ttt.hip"

namespace {

constexpr int PUCT_H_NODES = 0, PUCT_H_SIMS = 1, PUCT_H_PATH = 2, PUCT_H_LEAF = 3, PUCT_H_MOVER0 = 4, PUCT_H_LEAF_E = 5,
              PUCT_H_LEAF_MOVER = 6, PUCT_H_OCC = 8;
constexpr int PUCT_HDR_BYTES = 64, PUCT_PATH_SLOTS = 40, PUCT_FIXED_BYTES = PUCT_HDR_BYTES + 2 * PUCT_PATH_SLOTS;
constexpr uint32_t PUCT_PENDING = 1u, PUCT_TERMINAL = 2u;
constexpr int PUCT_MAX_S = 4095;
static_assert(PUCT_H_OCC + CRL_TTT_MAX_P <= PUCT_HDR_BYTES / 4 && PUCT_FIXED_BYTES % 16 == 0 && PUCT_PATH_SLOTS >= 33, "a tree's fixed part");

// bytes of one tree of S_cap + 1 nodes (host and device agree on it here and nowhere else)
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

// the maximum / the sum of v over the 64 lanes, in every lane: ttt_wave_max's DPP steps (ttt.hip), a lane without a source
// sees 0.  Every lane of the wave must run them.
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

// (the row_shr steps leave an inclusive prefix sum in each row of 16, the two broadcasts add the rows below: lane 63 holds all)
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

// floor(num / den) for num < 2^52 and 1 <= den < 2^32 (the double quotient is within one of it, the remainder decides) and
// the exact floor square root of x < 2^52: ttt_mcts_div / ttt_mcts_isqrt of ttt.hip
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

// a wave-uniform word in a vector register (ttt_in_vgpr of ttt.hip)
__device__ __forceinline__ uint32_t puct_in_vgpr(const uint32_t x)
{
    uint32_t v;
    asm("v_mov_b32 %0, %1" : "=v"(v) : "s"(x));
    return v;
}

// ---- begin: the header and the root of every tree; lane i < 16 writes header word i, the lanes of the cells clear the root's slots
__global__ void __launch_bounds__(256)
ttt_puct_begin_kernel(const int P, const int cells, const uint32_t full, const int64_t B, const uint32_t *__restrict__ occ,
                      const int8_t *__restrict__ winner, const int8_t *__restrict__ to_move, uint8_t *__restrict__ trees,
                      const uint64_t tree_bytes, const int S_cap)
{
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    for (int64_t b = (int64_t)blockIdx.x * 4 + wave; b < B; b += (int64_t)gridDim.x * 4) {
        const puct_tree t = puct_tree_of(trees, b, tree_bytes, S_cap, cells);
        uint32_t all = 0;
        for (int p = 0; p < P; ++p) all |= occ[p * B + b];
        const int w0 = winner[b], tm0 = to_move[b];
        const bool skipped = w0 >= 0 || (all & full) == full || (unsigned)tm0 >= (unsigned)P;
        uint32_t word = 0;
        if (lane == PUCT_H_NODES) word = skipped ? 0u : 1u;
        if (lane == PUCT_H_MOVER0) word = skipped ? 0u : (uint32_t)tm0;
        if (lane >= PUCT_H_OCC && lane < PUCT_H_OCC + P) word = occ[(int64_t)(lane - PUCT_H_OCC) * B + b];
        if (lane < PUCT_HDR_BYTES / 4) t.hdr[lane] = word;
        if (lane < PUCT_PATH_SLOTS) t.path[lane] = 0;
        if (lane == 0) { t.n[0] = 0u; t.w[0] = 0u; }
        if (lane < cells) { t.prior[lane] = 0; t.child[lane] = 0; }
    }
}

// ---- select: one descent of every tree, the leaf out in observation layout.  The lanes are the cells; the position is P
// words every lane holds alike; what the loop branches on goes through v_readfirstlane.
template <int P, int ND>
__global__ void __launch_bounds__(256)
ttt_puct_select_kernel(const ttt_dirs dd_arg, const int64_t B, uint8_t *__restrict__ trees, const uint64_t tree_bytes, const int S_cap,
                       const uint32_t cpuct, const uint32_t fpu, const int rel_mod, int8_t *__restrict__ board,
                       uint32_t *__restrict__ valid, int8_t *__restrict__ mover_g, uint8_t *__restrict__ pending_g,
                       uint32_t *__restrict__ leaf_occ)
{
    // the strides and start masks of the line test move into vector registers, alike in every lane, as ttt_mcts_kernel moves
    // them, where they would not fit beside the rest: left where the arguments arrive the 13-direction instances spilled 30
    // scalar registers and the 4-direction ones of six to eight players 2, 4 and 9
    ttt_dirs dd = dd_arg;
    if (ND > 4 || P > 5) {
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            dd.stride[d] = (int32_t)puct_in_vgpr((uint32_t)dd_arg.stride[d]);
            dd.start[d] = puct_in_vgpr(dd_arg.start[d]);
        }
    }
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const int cells = dd.n_cells;
    const bool cell_lane = lane < cells;
    for (int64_t b = (int64_t)blockIdx.x * 4 + wave; b < B; b += (int64_t)gridDim.x * 4) {
        const puct_tree t = puct_tree_of(trees, b, tree_bytes, S_cap, cells);
        uint32_t nn =(uint32_t)__builtin_amdgcn_readfirstlane((int)t.hdr[PUCT_H_NODES]);
        const uint32_t sims = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.hdr[PUCT_H_SIMS]);
        uint32_t o[P];
#pragma unroll
        for (int p = 0; p < P; ++p) o[p] = 0u;
        int tm = -1;
        uint32_t E = 0;
        bool pend = false;
        if (nn != 0u && nn <= (uint32_t)S_cap + 1u) {            // (a skipped tree is left alone)
            bool descend = sims < (uint32_t)S_cap;
            int w = -1, v = 0, d = 0, term = 0, ws = -1, rw;
            uint32_t path = 0;                                   // lane i: the node at depth i
            if (descend) {
#pragma unroll
                for (int p = 0; p < P; ++p) o[p] = t.hdr[PUCT_H_OCC + p];
                tm = (int)t.hdr[PUCT_H_MOVER0];
            }
            while (descend) {
                CRL_BOUNDS_LT(v, S_cap + 1, 230);
                const uint32_t nv = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.n[v]);
                if (nv == 0u) { pend = true; break; }           // an unexpanded node: the pending leaf
                E = dd.full & ~ttt_union<P>(o);
                const bool in_e = lane < 32 && ((E >> (lane & 31)) & 1u);
                const size_t at = (size_t)v * (size_t)cells + (size_t)lane;
                const uint32_t pe = in_e ? t.prior[at] : 0u;
                uint32_t cu = in_e ? t.child[at] : 0u;
                CRL_BOUNDS_LT(cu, S_cap + 1, 231);
                cu = min(cu, (uint32_t)S_cap);
                const uint64_t rt = puct_isqrt((uint64_t)nv << 16);
                uint32_t key = 0;
                if (in_e) {
                    const uint32_t nu = cu ? t.n[cu] : 0u, wu = cu ? t.w[cu] : 0u;
                    const uint64_t exploit = nu ? puct_div(wu, nu) : (uint64_t)fpu;
                    const uint64_t explore = puct_div((uint64_t)cpuct * pe * rt, (1u + min(nu, 4095u)) << 16);   // (n <= S_cap: den < 2^32)
                    key = (uint32_t)(exploit + explore) + 1u;    // score < 2^16 + 2^30: 31 bits, no room for the cell beside it
                }
                const uint32_t top = puct_wave_max(key);         // (all lanes: outside the branch above)
                const unsigned long long at_top = __ballot(in_e && key == top);
                if (at_top == 0ull) break;                       // (never: a running position has an empty cell)
                const int e = (int)__builtin_ctzll(at_top);      // ties: the lowest cell
                int u = __builtin_amdgcn_readlane((int)cu, e);
                const bool fresh = u == 0;
                if (fresh) {
                    if (nn > (uint32_t)S_cap) break;             // (never: nodes <= simulations + 2 <= S_cap + 1)
                    u = (int)nn++;
                    CRL_BOUNDS_LT(u, S_cap + 1, 232);
                    if (lane == e) t.child[at] = (uint16_t)u;
                    if (cell_lane) {
                        t.prior[(size_t)u * (size_t)cells + (size_t)lane] = 0;
                        t.child[(size_t)u * (size_t)cells + (size_t)lane] = 0;
                    }
                    if (lane == 0) { t.n[u] = 0u; t.w[u] = 0u; }
                }
                d += 1;
                path = lane == d ? (uint32_t)u : path;
                ttt_step_core<P, ND>(dd, o, w, tm, e, rw, term, ws);
                term = __builtin_amdgcn_readfirstlane(term);     // (every lane played the same ply)
                ws = __builtin_amdgcn_readfirstlane(ws);
                if (term) break;
                if (fresh) { pend = true; break; }               // the new node is the leaf: nothing of it is read back
                if (d >= 32) break;                              // (never: a ply that fills the board is terminal)
                v = u;
            }
            const bool have = pend || term;
            CRL_BOUNDS_LT(d, PUCT_PATH_SLOTS, 233);
            if (have && lane <= d) t.path[lane] = (uint16_t)path;
            E = dd.full & ~ttt_union<P>(o);
            if (lane == 0) {
                t.hdr[PUCT_H_NODES] = nn;
                t.hdr[PUCT_H_PATH] = have ? (uint32_t)d + 1u : 0u;
                t.hdr[PUCT_H_LEAF] = (pend ? PUCT_PENDING : PUCT_TERMINAL) | ((uint32_t)(ws + 1) << 8);
                t.hdr[PUCT_H_LEAF_E] = E;
                t.hdr[PUCT_H_LEAF_MOVER] = (uint32_t)tm;
            }
        }
        // ---- the outputs: the pending leaf as its mover sees it (ttt_write_relative's rule, lane = cell), zeros for the rest
        if (cell_lane) {
            int c = 0;
            if (pend) {
                c = -1;
#pragma unroll
                for (int p = 0; p < P; ++p) c = ((o[p] >> (lane & 31)) & 1u) ? p : c;
                if (c >= 0) {
                    const int rr = (c - tm) % rel_mod;
                    c = rr < 0 ? rr + rel_mod : rr;
                }
            }
            board[b * cells + lane] = (int8_t)c;
        }
        if (leaf_occ != nullptr && lane < P) {
            uint32_t mine = 0;
#pragma unroll
            for (int p = 0; p < P; ++p) mine = (p == lane) ? o[p] : mine;
            leaf_occ[(int64_t)lane * B + b] = pend ? mine : 0u;
        }
        if (lane == 0) {
            valid[b] = pend ? E : 0u;
            mover_g[b] = (int8_t)(pend ? tm : -1);
            pending_g[b] = pend ? 1 : 0;
        }
    }
}

// ---- backup: the leaf's priors, then lane i adds to the node at depth i of the path (distinct nodes: no atomics)
__global__ void __launch_bounds__(256)
ttt_puct_backup_kernel(const int P, const int cells, const int64_t B, uint8_t *__restrict__ trees, const uint64_t tree_bytes,
                       const int S_cap, const uint16_t *__restrict__ prior_g, const int32_t *__restrict__ value_g)
{
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const bool cell_lane = lane < cells;
    for (int64_t b = (int64_t)blockIdx.x * 4 + wave; b < B; b += (int64_t)gridDim.x * 4) {
        const puct_tree t = puct_tree_of(trees, b, tree_bytes, S_cap, cells);
        const uint32_t nn = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.hdr[PUCT_H_NODES]);
        const int plen = __builtin_amdgcn_readfirstlane((int)t.hdr[PUCT_H_PATH]);
        if (nn == 0u || plen <= 0 || plen > 33) continue;        // skipped, or no path outstanding: left alone
        const uint32_t sims = t.hdr[PUCT_H_SIMS], leaf = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.hdr[PUCT_H_LEAF]);
        const int tm0 = (int)t.hdr[PUCT_H_MOVER0], m = (int)t.hdr[PUCT_H_LEAF_MOVER], ws = (int)(leaf >> 8) - 1;
        const bool pend = (leaf & 3u) == PUCT_PENDING;
        if (pend) {
            const uint32_t E = t.hdr[PUCT_H_LEAF_E];
            const bool in_e = lane < 32 && ((E >> (lane & 31)) & 1u);
            const uint32_t L = min((uint32_t)t.path[plen - 1], (uint32_t)S_cap);
            CRL_BOUNDS_LT(t.path[plen - 1], S_cap + 1, 234);
            const uint32_t pr = in_e ? prior_g[b * cells + lane] : 0u;
            const uint32_t sum = puct_wave_sum(pr);              // (all lanes) <= 32 * 65535
            const uint32_t n_e = max((uint32_t)__popc(E), 1u);
            uint32_t slot = 0;
            if (in_e) slot = (uint32_t)min((uint64_t)65535u, sum ? puct_div((uint64_t)pr << 16, sum) : puct_div(65536u, n_e));
            if (cell_lane) t.prior[(size_t)L * (size_t)cells + (size_t)lane] = (uint16_t)slot;
        }
        if (lane < plen) {
            CRL_BOUNDS_LT(t.path[lane], S_cap + 1, 235);
            const uint32_t node = min((uint32_t)t.path[lane], (uint32_t)S_cap);
            uint32_t add = 0;
            if (lane > 0) {
                const int q = (tm0 + lane - 1) % P;              // who moved into the node at depth `lane`
                if (pend) {
                    const int j = (q - m + P) % P;
                    CRL_BOUNDS_LT(j, P, 236);
                    add = (uint32_t)min(max(value_g[b * P + j], 0), 65536);
                } else {
                    add = ws < 0 ? 32768u : (ws == q ? 65536u : 0u);
                }
            }
            t.n[node] += 1u;
            t.w[node] += add;
        }
        if (lane == 0) { t.hdr[PUCT_H_SIMS] = sims + 1u; t.hdr[PUCT_H_PATH] = 0u; }
    }
}

// ---- root: the root's children, its priors, the counts and the most visited cell (then the larger w, then the lowest cell)
__global__ void __launch_bounds__(256)
ttt_puct_root_kernel(const int cells, const int64_t B, uint8_t *__restrict__ trees, const uint64_t tree_bytes, const int S_cap,
                     uint32_t *__restrict__ visits, uint32_t *__restrict__ value, uint32_t *__restrict__ prior_out,
                     uint32_t *__restrict__ nodes, uint32_t *__restrict__ sims_out, int32_t *__restrict__ best)
{
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const bool cell_lane = lane < cells;
    for (int64_t b = (int64_t)blockIdx.x * 4 + wave; b < B; b += (int64_t)gridDim.x * 4) {
        const puct_tree t = puct_tree_of(trees, b, tree_bytes, S_cap, cells);
        const uint32_t nn = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.hdr[PUCT_H_NODES]);
        const bool live = nn != 0u;
        uint32_t cu = live && cell_lane ? t.child[lane] : 0u;
        CRL_BOUNDS_LT(cu, S_cap + 1, 237);
        cu = min(cu, (uint32_t)S_cap);
        const uint32_t vis = cu ? t.n[cu] : 0u, val = cu ? t.w[cu] : 0u;
        if (cell_lane) {
            visits[b * cells + lane] = vis;
            value[b * cells + lane] = val;
            prior_out[b * cells + lane] = live ? t.prior[lane] : 0u;
        }
        const uint32_t top_n = puct_wave_max(vis);               // (all lanes)
        const bool most = vis != 0u && vis == top_n;
        const uint32_t top_w = puct_wave_max(most ? val + 1u : 0u);
        const unsigned long long pick = __ballot(most && val + 1u == top_w);
        if (lane == 0) {
            nodes[b] = nn;
            sims_out[b] = live ? t.hdr[PUCT_H_SIMS] : 0u;
            best[b] = pick ? (int32_t)__builtin_ctzll(pick) : -1;
        }
    }
}

inline unsigned puct_blocks(const int64_t B)
{
    const uint64_t want = ((uint64_t)B + 3u) / 4u;
    return (unsigned)(want < (1u << 20) ? want : (1u << 20));    // (a grid-stride loop past that)
}

} // namespace

// the checks every entry shares: the context, B, the tree pointer, S_cap and the flags
#define PUCT_CHECK(fn)                                                                                                 \
    TTT_CTX_CHECK(fn);                                                                                                 \
    CRL_REQUIRE(tree != nullptr, "%s: NULL tree pointer", fn);                                                         \
    CRL_REQUIRE((((uintptr_t)tree) & 15) == 0, "%s: tree must be 16-byte aligned", fn);                                \
    CRL_REQUIRE(S_cap >= 1 && S_cap <= PUCT_MAX_S, "%s: S_cap=%d out of range 1..%d", fn, S_cap, PUCT_MAX_S);          \
    CRL_REQUIRE(ctx->ttt.n_cells >= ctx->ttt.P, "%s: a board of %d cells for %d players (as crl_ttt_playout)", fn,     \
                ctx->ttt.n_cells, ctx->ttt.P);                                                                         \
    const int cells = ctx->ttt.n_cells;                                                                                \
    const uint64_t tree_bytes = puct_tree_bytes(S_cap, cells);                                                         \
    uint8_t *trees = static_cast<uint8_t *>(tree)

int crl_ttt_puct_bounds(unsigned int *out4)
{
    CRL_BOUNDS_READBACK(out4);
    return CRL_OK;
}

extern "C" {

int64_t crl_ttt_puct_tree_bytes(const crl_ctx *ctx, int S_cap)
{
    CRL_REQUIRE(ctx != nullptr && ctx->game == CRL_GAME_TTT, "crl_ttt_puct_tree_bytes: ctx is not a tictactoe context");
    CRL_REQUIRE(S_cap >= 1 && S_cap <= PUCT_MAX_S, "crl_ttt_puct_tree_bytes: S_cap=%d out of range 1..%d", S_cap, PUCT_MAX_S);
    return (int64_t)puct_tree_bytes(S_cap, ctx->ttt.n_cells);
}

int crl_ttt_puct_begin(const crl_ctx *ctx, int64_t B, const uint32_t *occ, const int8_t *winner, const int8_t *to_move, int S_cap,
                       void *tree, void *stream)
{
    PUCT_CHECK("crl_ttt_puct_begin");
    CRL_REQUIRE(occ && winner && to_move, "crl_ttt_puct_begin: NULL state pointer");
    TTT_LAUNCH(ttt_puct_begin_kernel, puct_blocks(B), ctx->ttt.P, cells, ctx->ttt.full, B, occ, winner, to_move, trees, tree_bytes,
               S_cap);
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

int crl_ttt_puct_select(const crl_ctx *ctx, int64_t B, void *tree, int S_cap, uint32_t cpuct, uint32_t fpu, int rel_mod,
                        int8_t *board, uint32_t *valid, int8_t *mover, uint8_t *pending, uint32_t *leaf_occ, uint32_t flags,
                        void *stream)
{
    PUCT_CHECK("crl_ttt_puct_select");
    CRL_REQUIRE(board && valid && mover && pending, "crl_ttt_puct_select: NULL output pointer");
    CRL_REQUIRE(cpuct <= 65535u, "crl_ttt_puct_select: cpuct=%u out of range 0..65535", cpuct);
    CRL_REQUIRE(fpu <= 65536u, "crl_ttt_puct_select: fpu=%u out of range 0..65536", fpu);
    CRL_REQUIRE(rel_mod >= 1, "crl_ttt_puct_select: rel_mod must be >= 1 (as crl_ttt_board with a player)");
    CRL_REQUIRE(flags == 0, "crl_ttt_puct_select: unknown flags 0x%x", flags);
    const ttt_dirs dd = ctx->ttt_dd;
    TTT_DISPATCH_ND(ctx, TTT_LAUNCH((ttt_puct_select_kernel<PP, NDD>), puct_blocks(B), dd, B, trees, tree_bytes, S_cap, cpuct, fpu,
                                    rel_mod, board, valid, mover, pending, leaf_occ));
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

int crl_ttt_puct_backup(const crl_ctx *ctx, int64_t B, void *tree, int S_cap, const uint16_t *prior, const int32_t *value,
                        uint32_t flags, void *stream)
{
    PUCT_CHECK("crl_ttt_puct_backup");
    CRL_REQUIRE(prior && value, "crl_ttt_puct_backup: NULL input pointer");
    CRL_REQUIRE(flags == 0, "crl_ttt_puct_backup: unknown flags 0x%x", flags);
    TTT_LAUNCH(ttt_puct_backup_kernel, puct_blocks(B), ctx->ttt.P, cells, B, trees, tree_bytes, S_cap, prior, value);
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

int crl_ttt_puct_root(const crl_ctx *ctx, int64_t B, void *tree, int S_cap, uint32_t *visits, uint32_t *value, uint32_t *prior,
                      uint32_t *nodes, uint32_t *sims, int32_t *best, void *stream)
{
    PUCT_CHECK("crl_ttt_puct_root");
    CRL_REQUIRE(visits && value && prior && nodes && sims && best, "crl_ttt_puct_root: NULL output pointer");
    TTT_LAUNCH(ttt_puct_root_kernel, puct_blocks(B), cells, B, trees, tree_bytes, S_cap, visits, value, prior, nodes, sims, best);
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

} // extern "C"
