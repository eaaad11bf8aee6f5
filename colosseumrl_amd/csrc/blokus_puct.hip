// blokus_puct.hip -- tree search valued by the caller's network for Blokus (crl_blokus_puct_*; the contract is in
// include/colosseum_hip.h), gfx950, wave64.  The rules, the tables and the per-wave working set are blokus.hip's, taken in by
// including that file up to its kernels; the score arithmetic is blokus_mcts_search.hpp's.  The search is a translation unit
// of its own so that blokus.hip's kernels stay what they are.
//
// The trees live in the caller's buffer in HBM between the launches, one wave per tree in every kernel.  A node has at most
// W <= 64 children, the SAMPLED candidates of its position, so the wave's lanes are the children.  A tree of N = S_cap + 1
// nodes is, in bytes:
//   [0, 64)       16 header words: node count, simulation count, path length (0 = no path outstanding), leaf word
//                 (kind | winners mask << 8), the leaf's mover, the root's round, the root's mover, tcount, g, seed lo, seed hi
//   [64, 416)     the root position: 80 occupancy words, 4 inventories, 4 scores
//   [416, 1104)   the path, uint16 [344]: the node at each depth (at most 338 are used)
//   then          n uint32 [N], w uint32 [N], kt uint32 [N] (K | terminal << 8), id int32 [N][W], prior uint16 [N][W],
//                 child uint16 [N][W] (0 = none)
// rounded up to 16 bytes.  A node's ids, priors and child slots are contiguous, so a level of the descent is one load of each by
// the lanes k < K, and each lane gathers n and w of its own child.
// "Expanded" has no bit of its own: a descent only ever stands on the root or on a node it reached by a ply that did not end
// the game, and such a node has priors exactly when a backup has passed through it, which is n > 0.
// No lane reads through memory what another lane of the same launch wrote: a fresh node is the leaf, the candidates of a
// pending leaf go to the tree and to `cand` and are not read back, the path is written by select and read by backup, a launch
// later.  Every index read out of the tree is clamped before it addresses anything: a buffer that was never given to
// crl_blokus_puct_begin cannot make a kernel write outside it.
#define BLK_DEVICE_ONLY
#include "blokus.hip"
#include "blokus_mcts_search.hpp"

namespace {

constexpr int BP_H_NODES = 0, BP_H_SIMS = 1, BP_H_PATH = 2, BP_H_LEAF = 3, BP_H_LEAF_MOVER = 4, BP_H_ROUND = 5, BP_H_MOVER0 = 6,
              BP_H_TCOUNT = 7, BP_H_G = 8, BP_H_SEED_LO = 9, BP_H_SEED_HI = 10;
constexpr int BP_HDR_BYTES = 64, BP_STATE_WORDS = 4 * BN + 8, BP_PATH_SLOTS = 344, BP_MAX_DEPTH = 337;
constexpr int BP_FIXED_BYTES = BP_HDR_BYTES + 4 * BP_STATE_WORDS + 2 * BP_PATH_SLOTS;
constexpr uint32_t BP_PENDING = 1u, BP_TERMINAL = 2u;
constexpr int BP_MAX_S = 4095;
static_assert(BP_FIXED_BYTES == 1104 && BP_FIXED_BYTES % 16 == 0 && BP_PATH_SLOTS >= BP_MAX_DEPTH + 1, "a tree's fixed part");

// The window x pattern enumeration of blokus_list_kernel, restated (its declarations sit in blokus.hip's kernel section, which
// this unit does not compile): the pattern table behind the context's tables, {rows -4..-2, -1..1, 2..4, id part} per (piece,
// orientation, shift), and 128 anchors per chunk of a wave's window table.
constexpr int BP_WT = 128;
// The two forms of the pick meet here: up to this many candidates a leaf takes them by one blk_select walk each, above it by
// the one enumeration pass (measured; -DBP_SERIAL_MAX_K=0 / =64 build either form alone for the A/B).
#ifndef BP_SERIAL_MAX_K
#define BP_SERIAL_MAX_K 10
#endif
constexpr size_t BP_PAT_OFFSET = (sizeof(BlkTables) + 15) & ~(size_t)15;
constexpr int BP_PATTERNS = NPIECE * 40;
static_assert(sizeof(BlkTables) + 4 * sizeof(WaveLds) + BP_PATTERNS * 16 + 4 * BP_WT * 16 <= 65536, "a workgroup's 64 KB of LDS");

// bytes of one tree of S_cap + 1 nodes of W slots (host and device agree on it here and nowhere else)
__host__ __device__ inline uint64_t bp_tree_bytes(const int S_cap, const int W)
{
    const uint64_t N = (uint64_t)S_cap + 1u;
    return ((uint64_t)BP_FIXED_BYTES + N * (12u + 8u * (uint64_t)W) + 15u) & ~(uint64_t)15u;
}

// One tree: its base and the arrays as 32-bit byte offsets from it (a tree is at most 2.2 MB).  Nine pointers cost eighteen
// scalar registers through the whole of select, which has none to spare; the base and five offsets cost seven.
template <typename T>
struct bp_arr {
    uint8_t *base;
    uint32_t off;
    __device__ __forceinline__ T &operator[](const uint32_t i) const
    {
        return *reinterpret_cast<T *>(base + (uint64_t)(off + i * (uint32_t)sizeof(T)));
    }
};

struct bp_tree {
    bp_arr<uint32_t> hdr, state;
    bp_arr<uint16_t> path;
    bp_arr<uint32_t> n, w, kt;
    bp_arr<int32_t> id;
    bp_arr<uint16_t> prior, child;
};

__device__ __forceinline__ bp_tree bp_tree_of(uint8_t *trees, const int64_t b, const uint64_t tree_bytes, const int S_cap, const int W)
{
    uint8_t *base = trees + (uint64_t)b * tree_bytes;
    const uint32_t N = (uint32_t)S_cap + 1u, NW = N * (uint32_t)W;
    bp_tree t;
    t.hdr = {base, 0u};
    t.state = {base, (uint32_t)BP_HDR_BYTES};
    t.path = {base, (uint32_t)(BP_HDR_BYTES + 4 * BP_STATE_WORDS)};
    t.n = {base, (uint32_t)BP_FIXED_BYTES};
    t.w = {base, (uint32_t)BP_FIXED_BYTES + 4u * N};
    t.kt = {base, (uint32_t)BP_FIXED_BYTES + 8u * N};
    t.id = {base, (uint32_t)BP_FIXED_BYTES + 12u * N};
    t.prior = {base, (uint32_t)BP_FIXED_BYTES + 12u * N + 4u * NW};
    t.child = {base, (uint32_t)BP_FIXED_BYTES + 12u * N + 6u * NW};
    return t;
}

// K of a node as the tree holds it, clamped to the slots a node has
__device__ __forceinline__ int bp_node_k(const bp_tree &t, const uint32_t node, const int W, const int lo)
{
    const int K = (int)((uint32_t)__builtin_amdgcn_readfirstlane((int)t.kt[node]) & 0xffu);
    CRL_BOUNDS_IN(K, lo, W + 1, 370);
    return min(max(K, lo), W);
}

// ---- begin: the header, the root position and the root of every tree
__global__ void __launch_bounds__(256)
blokus_puct_begin_kernel(const int64_t B, const uint32_t seed_lo, const uint32_t seed_hi, const uint64_t first_env_id,
                         const uint32_t *__restrict__ occ, const uint32_t *__restrict__ inv_g, const int32_t *__restrict__ score_g,
                         const int32_t *__restrict__ round_g, const int32_t *__restrict__ to_move_g,
                         const uint32_t *__restrict__ tcount, uint8_t *__restrict__ trees, const uint64_t tree_bytes,
                         const int S_cap, const int W)
{
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    for (int64_t b = (int64_t)blockIdx.x * 4 + wave; b < B; b += (int64_t)gridDim.x * 4) {
        const bp_tree t = bp_tree_of(trees, b, tree_bytes, S_cap, W);
        uint32_t word = 0;
        if (lane == BP_H_NODES) word = 1u;
        if (lane == BP_H_ROUND) word = (uint32_t)round_g[b];
        if (lane == BP_H_MOVER0) word = (uint32_t)to_move_g[b] & 3u;
        if (lane == BP_H_TCOUNT) word = tcount ? tcount[b] : 0u;
        if (lane == BP_H_G) word = (uint32_t)(first_env_id + (uint64_t)b);
        if (lane == BP_H_SEED_LO) word = seed_lo;
        if (lane == BP_H_SEED_HI) word = seed_hi;
        if (lane < BP_HDR_BYTES / 4) t.hdr[lane] = word;
        for (int i = lane; i < BP_STATE_WORDS; i += 64)
            t.state[i] = i < 4 * BN ? occ[b * 4 * BN + i] : (i < 4 * BN + 4 ? inv_g[b * 4 + i - 4 * BN] : (uint32_t)score_g[b * 4 + i - 4 * BN - 4]);
        for (int i = lane; i < BP_PATH_SLOTS; i += 64) t.path[i] = 0;
        if (lane == 0) { t.n[0] = 0u; t.w[0] = 0u; t.kt[0] = 0u; }
        if (lane < W) { t.id[lane] = -2; t.prior[lane] = 0; t.child[lane] = 0; }
    }
}

// ---- the candidates of a pending leaf: ONE enumeration of the mover's legal actions in reference order, window x pattern
// as blokus_list_kernel, which keeps the K actions whose ranks are the targets instead of storing every id.

// window table entries [0, round-up-to-8 of the chunk's anchors) for the anchors [lo, lo + BP_WT) of the player whose rows
// are acq (blk_prep's {allowed << 8, corner << 8}, index y + 4): blk_list_windows of blokus.hip
__device__ __forceinline__ void bp_windows(uint4 *wt, const uint2 *acq, const int lane, const uint32_t crow, const uint32_t row_start,
                                           const int lo, const int n_c)
{
    uint32_t *Ww = reinterpret_cast<uint32_t *>(wt);
    uint32_t m = crow, idx = row_start;                          // lane y < 20 hands out its row's anchors: (x, y) for now
    while (__builtin_amdgcn_ballot_w64(m != 0u) != 0ull) {
        if (m != 0u) {
            const int ax = __builtin_ctz(m);
            m &= m - 1u;
            const uint32_t k = idx - (uint32_t)lo;
            if (k < (uint32_t)BP_WT) Ww[k * 4 + 3] = (uint32_t)ax | ((uint32_t)lane << 8);
            CRL_BOUNDS_LT(ax, BN, 371);
            idx += 1u;
        }
    }
    wave_sync();
    const int padded = (n_c + 7) & ~7;
#pragma unroll
    for (int h = 0; h < BP_WT / 64; ++h) {
        const int k = h * 64 + lane;
        if (k < n_c) {
            const uint32_t xy = Ww[k * 4 + 3];
            const int ax = (int)(xy & 0xffu), ay = (int)(xy >> 8);
            uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
            for (int dy = 0; dy < 9; ++dy) {                     // acq[y + 4] holds row y << 8: window column dx is bit ax + dx + 8
                CRL_BOUNDS_LT(ay + dy, 32, 372);                 // padded rows -4 .. 27
                const uint32_t row = acq[ay + dy].x;
                w[dy / 3] |= ((row >> (ax + 4)) & 0x1ffu) << (9 * (dy % 3));
            }
            wt[k] = make_uint4(~w[0], ~w[1], ~w[2], (uint32_t)((ay * BN + ax) * 40));
        } else if (k < padded) {
            wt[k] = make_uint4(~0u, ~0u, ~0u, 0u);               // the tail of the last unit of 8: never legal
        }
    }
    wave_sync();
}

// what the pass carries from unit to unit, all wave-uniform: the legal actions passed so far, the next slot to fill and the
// rank that goes there (0xffffffff once every slot is filled)
struct BpPick { uint32_t base; int next; uint32_t want; };

// The units of one piece over one chunk of anchors, N = the piece's cells (blk_list_units' enumeration: pass s of a unit
// covers candidates s * 64 + lane of 8 anchors x 8 N (orientation, shift) pairs, in output order).  The targets are
// ascending (lane k of `tgt` holds the rank of slot k), so a cursor on the scalar unit replaces a search for the stratum:
// a pass of `cnt` legal lanes covers the ranks [base, base + cnt), and while the wanted rank lies in there the legal lane
// with that many legal lanes below it stores its id to the slot -- one scalar compare per pass that holds no target.
template <int N>
__device__ __forceinline__ void bp_pick_units(const uint4 *wt, const uint4 *__restrict__ Pp, const int lane, const int n_c,
                                              const uint32_t tgt, const int K, BpPick &pk, int32_t *__restrict__ cand_row,
                                              int32_t *__restrict__ id_row)
{
    uint4 pat[N];
    int slot[N];                                                 // anchor of the unit (0..7)
    int ln = lane;                                               // (opaque, as in blk_list_units: the decode is not hoisted)
    asm volatile("" : "+v"(ln));
#pragma unroll
    for (int s = 0; s < N; ++s) {
        const uint32_t item = (uint32_t)(s * 64) + (uint32_t)ln;
        const uint32_t a = item / (uint32_t)(8 * N);
        slot[s] = (int)a;
        CRL_BOUNDS_LT(a, 8u, 373);
        pat[s] = Pp[item - a * (uint32_t)(8 * N)];
    }
    for (int u = 0; u < n_c && pk.next < K; u += 8) {            // (every slot filled: nothing is left to find)
        uint4 w[N];                                              // the unit's window reads go out together
#pragma unroll
        for (int s = 0; s < N; ++s) {
            CRL_BOUNDS_LT(u + slot[s], BP_WT, 374);
            w[s] = wt[u + slot[s]];
        }
#pragma unroll
        for (int s = 0; s < N; ++s) {
            const bool legal = ((w[s].x & pat[s].x) | (w[s].y & pat[s].y) | (w[s].z & pat[s].z)) == 0u;
            const unsigned long long lm = __builtin_amdgcn_ballot_w64(legal);
            const uint32_t end = pk.base + (uint32_t)__builtin_popcountll(lm);
            if (pk.want < end) {
                const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(lm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)lm, 0u));
                const int32_t id = (int32_t)(w[s].w + pat[s].w);
                do {
                    CRL_BOUNDS_LT(pk.next, K, 375);
                    if (legal && pk.base + below == pk.want) { cand_row[pk.next] = id; id_row[pk.next] = id; }
                    pk.next += 1;
                    pk.want = pk.next < K ? (uint32_t)__builtin_amdgcn_readlane((int)tgt, pk.next) : 0xffffffffu;
                } while (pk.want < end);
            }
            pk.base = end;
        }
    }
}

// the K candidates of the leaf `v` whose mover q (rows L.ac[q] as blk_prep left them, inventory iq) has n_legal > 0 legal
// actions: slot k gets the action of rank tgt_k, in the tree's id row and in the caller's cand row
__device__ __forceinline__ void bp_pick(const WaveLds &L, uint4 *wt, const uint4 *Pt, const int lane, const int q, const uint32_t iq,
                                        const uint32_t piece_cells, const uint32_t tgt, const int K, int32_t *__restrict__ cand_row,
                                        int32_t *__restrict__ id_row)
{
    const uint32_t crow = lane < BN ? (L.ac[q][lane + 4].y >> 8) : 0u;
    const uint32_t crow_n = (uint32_t)__popc(crow);
    const uint32_t incl = wave_scan_incl(crow_n, lane);
    const int A = min(__builtin_amdgcn_readlane((int)incl, 63), BN * BN);
    const int nchunks = (A + BP_WT - 1) / BP_WT;                 // 1 unless a player has more than 128 anchors
    if (nchunks == 1) bp_windows(wt, L.ac[q], lane, crow, incl - crow_n, 0, A);
    BpPick pk = {0u, 0, (uint32_t)__builtin_amdgcn_readlane((int)tgt, 0)};
    for (int piece = 0; piece < NPIECE && pk.next < K; ++piece) {
        if (!((iq >> piece) & 1u)) continue;
        const int n = __builtin_amdgcn_readlane((int)piece_cells, piece);
        const uint4 *Pp = &Pt[piece * 40];
        for (int c = 0; c < nchunks; ++c) {
            const int n_c = A - c * BP_WT < BP_WT ? A - c * BP_WT : BP_WT;
            if (nchunks > 1) bp_windows(wt, L.ac[q], lane, crow, incl - crow_n, c * BP_WT, n_c);
            switch (n) {
                case 1: bp_pick_units<1>(wt, Pp, lane, n_c, tgt, K, pk, cand_row, id_row); break;
                case 2: bp_pick_units<2>(wt, Pp, lane, n_c, tgt, K, pk, cand_row, id_row); break;
                case 3: bp_pick_units<3>(wt, Pp, lane, n_c, tgt, K, pk, cand_row, id_row); break;
                case 4: bp_pick_units<4>(wt, Pp, lane, n_c, tgt, K, pk, cand_row, id_row); break;
                default: bp_pick_units<5>(wt, Pp, lane, n_c, tgt, K, pk, cand_row, id_row); break;
            }
        }
    }
}

// a wave-uniform word in a vector register (ttt_in_vgpr of ttt.hip): select parks its launch constants there, and with them
// the tree's base and array offsets, which are then computed on the vector unit -- held in scalar registers through the
// descent, the count pass and the pick they were 22 scalar spills
__device__ __forceinline__ uint32_t bp_in_vgpr(const uint32_t x)
{
    uint32_t v;
    asm("v_mov_b32 %0, %1" : "=v"(v) : "s"(x));
    return v;
}
__device__ __forceinline__ uint64_t bp_in_vgpr64(const uint64_t x)
{
    return ((uint64_t)bp_in_vgpr((uint32_t)(x >> 32)) << 32) | bp_in_vgpr((uint32_t)x);
}

// select's output pointers.  They are used once per tree, behind the descent and the pick; left where the arguments arrive
// they hold 28 scalar registers through all of it (the kernel then spilled 55), so the workgroup parks them in LDS and a wave
// reads them back where it writes a leaf out.
struct BpOut {
    int8_t *obs_board;
    uint8_t *obs_pieces;
    int32_t *obs_score, *cand, *n_cand, *n_legal;
    int8_t *mover;
    uint8_t *pending;
    uint32_t *depth, *leaf_occ, *leaf_inv;
    int32_t *leaf_score, *leaf_round, *leaf_to_move;
};

// ---- select: one descent of every tree, the leaf out in observation layout with its candidates beside it.  The board is in
// the wave's WaveLds, the inventories and scores in the lanes (lane & 3 = player) as in blk_mcts_search; while a node is
// scored lane k is its slot k; what the loop branches on goes through v_readfirstlane.
// (4 waves per SIMD: what the workgroup's 40 KB of LDS admit on a CU anyway)
__global__ void __launch_bounds__(256, 4)
blokus_puct_select_kernel(const BlkTables *__restrict__ tables, const int64_t B_arg, uint8_t *__restrict__ trees_arg,
                          const uint64_t tree_bytes_arg, const int S_cap_arg, const int W_arg, const uint32_t cpuct_arg,
                          const uint32_t fpu_arg, const BpOut out_arg)
{
    const int64_t B = (int64_t)bp_in_vgpr64((uint64_t)B_arg), stride = (int64_t)bp_in_vgpr(gridDim.x * 4u);
    const uint64_t tree_bytes = bp_in_vgpr64(tree_bytes_arg), trees_v = bp_in_vgpr64((uint64_t)(uintptr_t)trees_arg);
    const uint32_t cpuct = bp_in_vgpr(cpuct_arg), fpu = bp_in_vgpr(fpu_arg);
    const int S_cap_v = (int)bp_in_vgpr((uint32_t)S_cap_arg), W_v = (int)bp_in_vgpr((uint32_t)W_arg);
    __shared__ BpOut Out;
    if (threadIdx.x == 0) Out = out_arg;
    __shared__ uint4 Pt[BP_PATTERNS];
    __shared__ uint4 Wt[4][BP_WT];
    {
        const uint4 *pat = reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(tables) + BP_PAT_OFFSET);
        for (int i = threadIdx.x; i < BP_PATTERNS; i += blockDim.x) Pt[i] = pat[i];
    }
    BLK_WAVE_SETUP();                                            // (its barrier covers the pattern table too)
    const uint32_t piece_cells = lane < 24 ? T.ncell[lane] : 0u;
    const BlkOwners owners = blk_shape_owners(T, lane);
    uint32_t *flat = &L.occ[0][0];                               // the board's 80 row words: lane i holds words i and 64 + i
    for (int64_t b = (int64_t)blockIdx.x * 4 + wave_; b < B; b += stride) {
        uint8_t *trees = reinterpret_cast<uint8_t *>((uintptr_t)trees_v);
        // S_cap and W as the scalars the control flow wants; the tree's offsets come from the vector copies
        const int S_cap = __builtin_amdgcn_readfirstlane(S_cap_v), W = __builtin_amdgcn_readfirstlane(W_v);
        // (an opaque copy of the lane id per tree: with the launch's own, every lane predicate of the body is hoisted out of
        // the grid-stride loop into a scalar register pair, and the kernel spills 26 scalar registers to hold them)
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const bp_tree t = bp_tree_of(trees, b, tree_bytes, S_cap_v, W_v);
        uint32_t nn = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.hdr[BP_H_NODES]);
        CRL_BOUNDS_IN(nn, 1, S_cap + 2, 376);
        nn = min(max(nn, 1u), (uint32_t)S_cap + 1u);
        const uint32_t sims = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.hdr[BP_H_SIMS]);
        bool pend = false;
        int term = 0, d = 0, v = 0, pl = 0, round = 0, K = 0;
        uint32_t vinv = 0u, n_leg = 0u, winners = 0u;
        int vscore = 0;
        if (sims < (uint32_t)S_cap) {                            // (a tree at capacity is not descended)
            flat[ln] = t.state[ln];
            if (ln < 4 * BN - 64) flat[64 + ln] = t.state[64 + ln];
            vinv = t.state[4 * BN + (ln & 3)];
            vscore = (int)t.state[4 * BN + 4 + (ln & 3)];
            round = __builtin_amdgcn_readfirstlane((int)t.hdr[BP_H_ROUND]);
            pl = __builtin_amdgcn_readfirstlane((int)t.hdr[BP_H_MOVER0]) & 3;
            wave_sync();
            if (ln == 0) t.path[0] = 0;
            for (;;) {
                CRL_BOUNDS_LT(v, S_cap + 1, 377);
                const uint32_t nv = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.n[v]);
                if (nv == 0u) { pend = true; break; }           // an unexpanded node: the pending leaf
                const int Kv = bp_node_k(t, (uint32_t)v, W, 1);
                const bool mine = ln < Kv;
                const size_t at = (size_t)v * (size_t)W + (size_t)ln;
                const uint32_t pe = mine ? t.prior[at] : 0u;
                uint32_t cu = mine ? t.child[at] : 0u;
                const int cid = mine ? t.id[at] : -1;
                CRL_BOUNDS_LT(cu, S_cap + 1, 378);
                cu = min(cu, (uint32_t)S_cap);
                const uint64_t rt = blk_mcts_isqrt((uint64_t)nv << 16);
                uint32_t key = 0u;
                if (mine) {
                    const uint32_t nu = cu ? t.n[cu] : 0u, wu = cu ? t.w[cu] : 0u;
                    const uint64_t exploit = nu ? blk_mcts_div(wu, nu) : (uint64_t)fpu;
                    CRL_BOUNDS_LT(nu, 4096u, 383);               // (n <= S_cap <= 4095: the denominator stays below 2^32)
                    const uint64_t explore = blk_mcts_div((uint64_t)cpuct * pe * rt, (1u + min(nu, 4095u)) << 16);
                    key = (uint32_t)(exploit + explore) + 1u;    // score < 2^16 + 2^30: 31 bits
                }
                const uint32_t top = blk_wave_max(key);          // (all lanes: outside the branch above)
                const int e = (int)__builtin_ctzll(__ballot(mine && key == top) | (1ull << 63));   // ties: the lowest slot
                int u = __builtin_amdgcn_readlane((int)cu, e);
                int id = __builtin_amdgcn_readlane(cid, e);
                CRL_BOUNDS_IN(id, -1, ACTION_IDS, 379);
                id = id >= ACTION_IDS ? -1 : id;
                const bool fresh = u == 0;
                if (!fresh) {                                    // an existing child: its ply is legal here, as when it was made
                    term = (int)((((uint32_t)__builtin_amdgcn_readfirstlane((int)t.kt[u])) >> 8) & 1u);
                    if (id >= 0) {
                        const BlkMove mv = blk_decode(id);
                        const int n = __builtin_amdgcn_readlane((int)piece_cells, mv.piece);
                        blk_place_legal(T, L, pl, mv, ln, n);
                        const uint32_t left = vinv & ~(1u << mv.piece);  // ai.py:44-54 for the mover's ln(s)
                        const bool me = (ln & 3) == pl;
                        vscore += me ? n + (left == 0u ? (mv.piece == 0 ? 20 : 15) : 0) : 0;
                        vinv = me ? left : vinv;
                    }
                } else {                                         // a new child: the ply as crl_blokus_step plays it
                    if (nn > (uint32_t)S_cap) break;             // (never: nodes <= simulations + 2 <= S_cap + 1)
                    u = (int)nn++;
                    blk_prep(L, ln, round);                    // every player's rows of the PRE-move board (:424)
                    uint32_t inv[4];
                    int score[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        inv[q] = (uint32_t)__builtin_amdgcn_readlane((int)vinv, q);
                        score[q] = __builtin_amdgcn_readlane(vscore, q);
                    }
                    if (id >= 0) (void)blk_apply(T, L, pl, blk_decode(id), inv, score, ln);
                    term = blk_anyone_moves(T, L, inv, ln, &owners) ? 0 : 1;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        vinv = (ln & 3) == q ? inv[q] : vinv;
                        vscore = (ln & 3) == q ? score[q] : vscore;
                    }
                    if (ln == e) t.child[at] = (uint16_t)u;
                    if (ln == 0) { t.n[u] = 0u; t.w[u] = 0u; t.kt[u] = (uint32_t)term << 8; }
                }
                round = blk_next_round(round, pl);
                pl = blk_next_mover(pl);
                d += 1;
                if (ln == 0) t.path[d] = (uint16_t)u;
                v = u;
                if (term || d >= BP_MAX_DEPTH) break;            // (d >= 337: never, see the contract)
                if (fresh) { pend = true; break; }               // the new node is the leaf: nothing of it is read back
            }
        }
        int32_t *cand_row = Out.cand + b * W;
        if (pend) {
            // ---- the candidates of the leaf: the count, the K target ranks, one enumeration
            blk_prep(L, ln, round, pl);
            const uint32_t ip = (uint32_t)__builtin_amdgcn_readlane((int)vinv, pl);
            n_leg = blk_count(T, L, pl, ip, ln);
            K = n_leg == 0u ? 1 : (int)min(n_leg, (uint32_t)W);
            int32_t *id_row = &t.id[(uint32_t)v * (uint32_t)W];
            if (ln < W) {
                t.prior[(size_t)v * (size_t)W + ln] = 0;
                t.child[(size_t)v * (size_t)W + ln] = 0;
                if (ln >= K) { id_row[ln] = -2; cand_row[ln] = -2; }
            }
            if (n_leg == 0u) {
                if (ln == 0) { id_row[0] = -1; cand_row[0] = -1; }                 // the pass
            } else {
                uint32_t tgt = (uint32_t)ln;                   // L <= W: everything, slot = rank
                if (n_leg > (uint32_t)W && ln < K) {           // one rank from each of W strata
                    const uint32_t lo = (uint32_t)ln * n_leg / (uint32_t)W, hi = ((uint32_t)ln + 1u) * n_leg / (uint32_t)W;
                    const uint32_t tc = t.hdr[BP_H_TCOUNT];
                    const philox_out dr = philox4x32_10(t.hdr[BP_H_G], 0xC0000000u | (uint32_t)v,
                                                        0x80000000u | ((tc & 0x07FFFFFFu) << 4) | ((uint32_t)ln >> 2),
                                                        CRL_TAG_BLOKUS_PLAYOUT, t.hdr[BP_H_SEED_LO], t.hdr[BP_H_SEED_HI]);
                    const int ws = ln & 3;
                    const uint32_t uk = ws == 0 ? dr.w[0] : ws == 1 ? dr.w[1] : ws == 2 ? dr.w[2] : dr.w[3];
                    tgt = lo + __umulhi(uk, hi - lo);
                }
                if (K <= BP_SERIAL_MAX_K) {                      // few candidates: a rank walk each (blk_count filled pcnt)
                    for (int k = 0; k < K; ++k) {
                        const BlkMove mv = blk_select(T, L, pl, ip, (uint32_t)__builtin_amdgcn_readlane((int)tgt, k), ln);
                        if (ln == 0) { cand_row[k] = blk_encode(mv); id_row[k] = blk_encode(mv); }
                    }
                } else {
                    bp_pick(L, Wt[wave_], Pt, ln, pl, ip, piece_cells, tgt, K, cand_row, id_row);
                }
            }
            if (ln == 0) t.kt[v] = (uint32_t)K;                // (a pending leaf was not reached by a terminal ply)
        } else if (ln < W) {
            cand_row[ln] = -2;
        }
        // ---- the leaf out: the observation of its mover, the state rows; zeros for a tree without a pending leaf
        uint32_t inv[4];
        int score[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            inv[q] = (uint32_t)__builtin_amdgcn_readlane((int)vinv, q);
            score[q] = __builtin_amdgcn_readlane(vscore, q);
        }
        if (term) winners = (uint32_t)blk_outcome(false, 0, score).winners;
        const BpOut o = Out;
        if (pend) {
            blk_write_observation(L.occ, inv, score, pl, b, ln, o.obs_board, o.obs_pieces, o.obs_score);
        } else {
            for (int i = ln; i < BN * BN / 4; i += 64) reinterpret_cast<uint32_t *>(o.obs_board + b * (BN * BN))[i] = 0u;
            for (int i = ln; i < 4 * NPIECE; i += 64) o.obs_pieces[b * 4 * NPIECE + i] = 0;
            if (ln < 4) o.obs_score[b * 4 + ln] = 0;
        }
        if (o.leaf_occ != nullptr) {
            for (int i = ln; i < 4 * BN; i += 64) o.leaf_occ[b * 4 * BN + i] = pend ? flat[i] : 0u;
            if (ln < 4) {
                o.leaf_inv[b * 4 + ln] = pend ? vinv : 0u;
                o.leaf_score[b * 4 + ln] = pend ? vscore : 0;
            }
            if (ln == 0) { o.leaf_round[b] = pend ? round : 0; o.leaf_to_move[b] = pend ? pl : 0; }
        }
        if (ln == 0) {
            const bool have = pend || term;
            o.n_cand[b] = K;
            o.n_legal[b] = (int32_t)n_leg;
            o.mover[b] = (int8_t)(pend ? pl : -1);
            o.pending[b] = pend ? 1 : 0;
            o.depth[b] = pend ? (uint32_t)d : 0u;
            t.hdr[BP_H_NODES] = nn;
            t.hdr[BP_H_PATH] = have ? (uint32_t)d + 1u : 0u;
            t.hdr[BP_H_LEAF] = (pend ? BP_PENDING : BP_TERMINAL) | (winners << 8);
            t.hdr[BP_H_LEAF_MOVER] = (uint32_t)pl;
        }
        wave_sync();                                             // (the next tree's board goes where this one's was read)
    }
}

// ---- backup: the leaf's priors over its K candidates, then lane i adds to the nodes at depths i, i + 64, ... of the path
// (distinct nodes: no atomics)
__global__ void __launch_bounds__(256)
blokus_puct_backup_kernel(const int64_t B, uint8_t *__restrict__ trees, const uint64_t tree_bytes, const int S_cap, const int W,
                          const uint16_t *__restrict__ prior_g, const int32_t *__restrict__ value_g)
{
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    for (int64_t b = (int64_t)blockIdx.x * 4 + wave; b < B; b += (int64_t)gridDim.x * 4) {
        const bp_tree t = bp_tree_of(trees, b, tree_bytes, S_cap, W);
        const int plen = __builtin_amdgcn_readfirstlane((int)t.hdr[BP_H_PATH]);
        if (plen <= 0 || plen > BP_MAX_DEPTH + 1) continue;      // no path outstanding: left alone
        const uint32_t sims = t.hdr[BP_H_SIMS], leaf = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.hdr[BP_H_LEAF]);
        const int pl0 = (int)(t.hdr[BP_H_MOVER0] & 3u), m = (int)(t.hdr[BP_H_LEAF_MOVER] & 3u);
        const bool pend = (leaf & 3u) == BP_PENDING;
        uint32_t val[4];                                         // of player q
        if (pend) {
            CRL_BOUNDS_LT(t.path[plen - 1], S_cap + 1, 380);
            const uint32_t node = min((uint32_t)__builtin_amdgcn_readfirstlane((int)t.path[plen - 1]), (uint32_t)S_cap);
            const int K = bp_node_k(t, node, W, 1);
            const uint32_t pr = lane < K ? prior_g[b * W + lane] : 0u;
            const uint32_t sum = (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_incl(pr, lane), 63);   // (all lanes) <= 64 * 65535
            if (lane < K) {
                const uint64_t slot = sum ? blk_mcts_div((uint64_t)pr << 16, sum) : blk_mcts_div(65536u, (uint32_t)K);
                t.prior[(size_t)node * (size_t)W + (size_t)lane] = (uint16_t)min((uint64_t)65535u, slot);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) val[q] = (uint32_t)min(max(value_g[b * 4 + ((q - m) & 3)], 0), 65536);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) val[q] = ((leaf >> (8 + q)) & 1u) ? 65536u : 0u;
        }
        for (int i = lane; i < plen; i += 64) {
            CRL_BOUNDS_LT(t.path[i], S_cap + 1, 381);
            const uint32_t node = min((uint32_t)t.path[i], (uint32_t)S_cap);
            const int q = (pl0 + i - 1) & 3;                     // who moved into the node at depth i
            uint32_t add = 0u;
#pragma unroll
            for (int p = 0; p < 4; ++p) add = (p == q) ? val[p] : add;
            t.n[node] += 1u;
            if (i > 0) t.w[node] += add;
        }
        if (lane == 0) { t.hdr[BP_H_SIMS] = sims + 1u; t.hdr[BP_H_PATH] = 0u; }
    }
}

// ---- root: lane k is the root's slot k; the most visited child (then the larger w, then the lowest slot)
__global__ void __launch_bounds__(256)
blokus_puct_root_kernel(const int64_t B, uint8_t *__restrict__ trees, const uint64_t tree_bytes, const int S_cap, const int W,
                        int32_t *__restrict__ ids, uint32_t *__restrict__ visits, uint32_t *__restrict__ value,
                        uint32_t *__restrict__ prior_out, uint32_t *__restrict__ nodes, uint32_t *__restrict__ sims_out,
                        int32_t *__restrict__ best)
{
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    for (int64_t b = (int64_t)blockIdx.x * 4 + wave; b < B; b += (int64_t)gridDim.x * 4) {
        const bp_tree t = bp_tree_of(trees, b, tree_bytes, S_cap, W);
        const bool expanded = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.n[0]) != 0u;
        const int K = expanded ? bp_node_k(t, 0u, W, 0) : 0;
        const bool mine = lane < K;
        uint32_t cu = mine ? t.child[lane] : 0u;
        CRL_BOUNDS_LT(cu, S_cap + 1, 382);
        cu = min(cu, (uint32_t)S_cap);
        const uint32_t vis = cu ? t.n[cu] : 0u, val = cu ? t.w[cu] : 0u;
        const int cid = mine ? t.id[lane] : -2;
        if (lane < W) {
            ids[b * W + lane] = cid;
            visits[b * W + lane] = vis;
            value[b * W + lane] = val;
            prior_out[b * W + lane] = mine ? t.prior[lane] : 0u;
        }
        const uint32_t top_n = blk_wave_max(vis);                // (all lanes)
        const bool most = vis != 0u && vis == top_n;
        const uint32_t top_w = blk_wave_max(most ? val + 1u : 0u);
        const unsigned long long pick = __ballot(most && val + 1u == top_w);
        const int best_id = pick ? __builtin_amdgcn_readlane(cid, (int)__builtin_ctzll(pick)) : -2;
        if (lane == 0) {
            nodes[b] = t.hdr[BP_H_NODES];
            sims_out[b] = t.hdr[BP_H_SIMS];
            best[b] = best_id;
        }
    }
}

inline unsigned bp_blocks(const int64_t B)
{
    const uint64_t want = ((uint64_t)B + 3u) / 4u;
    return (unsigned)(want < (1u << 20) ? want : (1u << 20));    // (a grid-stride loop past that)
}

} // namespace

// the checks every entry shares: B, the tree pointer, S_cap, W and, last, the context
#define BP_CHECK(fn)                                                                                                   \
    CRL_REQUIRE(tree != nullptr, fn ": NULL tree pointer");                                                            \
    CRL_REQUIRE((((uintptr_t)tree) & 15) == 0, fn ": tree must be 16-byte aligned");                                   \
    CRL_REQUIRE(B > 0 && B <= ((int64_t)1 << 28), fn ": B=%lld out of range", (long long)B);                           \
    CRL_REQUIRE(S_cap >= 1 && S_cap <= BP_MAX_S, fn ": S_cap=%d out of range 1..%d", S_cap, BP_MAX_S);                 \
    CRL_REQUIRE(W >= 1 && W <= 64, fn ": W=%d out of range 1..64", W);                                                 \
    CRL_REQUIRE(ctx != nullptr && ctx->game == CRL_GAME_BLOKUS && ctx->blokus, fn ": ctx is not a blokus context");    \
    const uint64_t tree_bytes = bp_tree_bytes(S_cap, W);                                                               \
    uint8_t *trees = static_cast<uint8_t *>(tree)

int crl_blokus_puct_bounds(unsigned int *out4)
{
    CRL_BOUNDS_READBACK(out4);
    return CRL_OK;
}

extern "C" {

int64_t crl_blokus_puct_tree_bytes(const crl_ctx *ctx, int S_cap, int W)
{
    CRL_REQUIRE(ctx != nullptr && ctx->game == CRL_GAME_BLOKUS && ctx->blokus, "crl_blokus_puct_tree_bytes: ctx is not a blokus context");
    CRL_REQUIRE(S_cap >= 1 && S_cap <= BP_MAX_S, "crl_blokus_puct_tree_bytes: S_cap=%d out of range 1..%d", S_cap, BP_MAX_S);
    CRL_REQUIRE(W >= 1 && W <= 64, "crl_blokus_puct_tree_bytes: W=%d out of range 1..64", W);
    return (int64_t)bp_tree_bytes(S_cap, W);
}

int crl_blokus_puct_begin(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, const uint32_t *occ,
                          const uint32_t *inv, const int32_t *score, const int32_t *round, const int32_t *to_move,
                          const uint32_t *tcount, int S_cap, int W, void *tree, void *stream)
{
    CRL_REQUIRE(occ && inv && score && round && to_move, "crl_blokus_puct_begin: NULL state pointer");
    BP_CHECK("crl_blokus_puct_begin");
    hipLaunchKernelGGL(blokus_puct_begin_kernel, dim3(bp_blocks(B)), dim3(256), 0, (hipStream_t)stream, B, (uint32_t)seed,
                       (uint32_t)(seed >> 32), first_env_id, occ, inv, score, round, to_move, tcount, trees, tree_bytes, S_cap, W);
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

int crl_blokus_puct_select(const crl_ctx *ctx, int64_t B, void *tree, int S_cap, int W, uint32_t cpuct, uint32_t fpu,
                           int8_t *obs_board, uint8_t *obs_pieces, int32_t *obs_score, int32_t *cand, int32_t *n_cand,
                           int32_t *n_legal, int8_t *mover, uint8_t *pending, uint32_t *depth,
                           uint32_t *leaf_occ, uint32_t *leaf_inv, int32_t *leaf_score, int32_t *leaf_round, int32_t *leaf_to_move,
                           uint32_t flags, void *stream)
{
    CRL_REQUIRE(obs_board && obs_pieces && obs_score && cand && n_cand && n_legal && mover && pending && depth,
                "crl_blokus_puct_select: NULL output pointer");
    const int n_leaf = (leaf_occ != nullptr) + (leaf_inv != nullptr) + (leaf_score != nullptr) + (leaf_round != nullptr) +
                       (leaf_to_move != nullptr);
    CRL_REQUIRE(n_leaf == 0 || n_leaf == 5, "crl_blokus_puct_select: the leaf_* pointers must be all NULL or all set");
    CRL_REQUIRE(cpuct <= 65535u, "crl_blokus_puct_select: cpuct=%u out of range 0..65535", cpuct);
    CRL_REQUIRE(fpu <= 65536u, "crl_blokus_puct_select: fpu=%u out of range 0..65536", fpu);
    CRL_REQUIRE(flags == 0, "crl_blokus_puct_select: unknown flags 0x%x", flags);
    BP_CHECK("crl_blokus_puct_select");
    const BpOut out = {obs_board, obs_pieces, obs_score, cand, n_cand, n_legal, mover, pending, depth, leaf_occ, leaf_inv, leaf_score,
                       leaf_round, leaf_to_move};
    hipLaunchKernelGGL(blokus_puct_select_kernel, dim3(bp_blocks(B)), dim3(256), 0, (hipStream_t)stream,
                       (const BlkTables *)ctx->blokus, B, trees, tree_bytes, S_cap, W, cpuct, fpu, out);
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

int crl_blokus_puct_backup(const crl_ctx *ctx, int64_t B, void *tree, int S_cap, int W, const uint16_t *prior, const int32_t *value,
                           uint32_t flags, void *stream)
{
    CRL_REQUIRE(prior && value, "crl_blokus_puct_backup: NULL input pointer");
    CRL_REQUIRE(flags == 0, "crl_blokus_puct_backup: unknown flags 0x%x", flags);
    BP_CHECK("crl_blokus_puct_backup");
    hipLaunchKernelGGL(blokus_puct_backup_kernel, dim3(bp_blocks(B)), dim3(256), 0, (hipStream_t)stream, B, trees, tree_bytes,
                       S_cap, W, prior, value);
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

int crl_blokus_puct_root(const crl_ctx *ctx, int64_t B, void *tree, int S_cap, int W, int32_t *ids, uint32_t *visits,
                         uint32_t *value, uint32_t *prior, uint32_t *nodes, uint32_t *sims, int32_t *best, void *stream)
{
    CRL_REQUIRE(ids && visits && value && prior && nodes && sims && best, "crl_blokus_puct_root: NULL output pointer");
    BP_CHECK("crl_blokus_puct_root");
    hipLaunchKernelGGL(blokus_puct_root_kernel, dim3(bp_blocks(B)), dim3(256), 0, (hipStream_t)stream, B, trees, tree_bytes, S_cap,
                       W, ids, visits, value, prior, nodes, sims, best);
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

} // extern "C"
