// tron_territory.hip -- Voronoi territory for Tron positions (crl_tron_territory) and the territory-greedy scripted agent
// (crl_tron_sample_territory).  Contract: include/colosseum_hip.h; DESIGN.md section 4.1b.
//
// Both calls run the same level-synchronous multi-source flood on occupancy bitboards.  With `nw[p]` the cells player p
// reaches at the current distance (level 1: its first cells), one level is
//     contested = cells in two or more nw[p];   area[p] += popcount(nw[p] & ~contested);
//     free &= ~(union of nw[p]);                nw[p] = expand(nw[p]) & free
// Contested cells stay in the frontiers (ties propagate) and a claimed cell is never entered again: a player that arrives
// at a claimed cell later can neither win nor tie anything beyond it, so flooding only through unclaimed cells is exact.
// Every level with a new bit claims at least one cell, so a flood has at most N*N levels; the loops carry that bound.
//
// Boards up to 64x64, the register kernels: one lane per board ROW, the row one 32- or 64-bit word, floor(64 / N)
// instances on consecutive lane groups of a wave.  Horizontal neighbours are shifts; vertical ones come from lane +- 1 by
// DPP wave shifts (full-rate VALU moves, no LDS traffic: a ds_bpermute per dword, direction and player would put 8-32 LDS
// operations into every level of a loop that is one dependent chain), masked at the instances' first and last rows.  The P
// frontiers and the per-lane area sums stay in registers; one segmented shuffle reduction per instance at the end.  The
// level loop ends when a wave-wide ballot sees no new bit.
// Boards 65..181 wide, the LDS kernels: one workgroup per instance, free + P frontier bitboards in LDS with rows padded to
// whole 32-bit words, threads over words, two barriers per level.  Correct, not tuned.
#include "crl_common.hpp"

namespace {

// bits 0..3: bytes 0..3 of x are non-zero (an occupied cell: any value but 0)
__device__ __forceinline__ uint32_t terr_nz_nibble(const uint32_t x)
{
    const uint32_t m = (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
    return (((m >> 7) * 0x00204081u) >> 21) & 0xfu;
}

// occupancy of the n <= 64 cells from p on: bit i set iff p[i] != 0.  Aligned dword loads, each holding at least one byte
// of the run (so none leaves the pages the run lies in).
__device__ __forceinline__ uint64_t terr_occ_run(const int8_t *p, const int n)
{
    const uintptr_t addr = reinterpret_cast<uintptr_t>(p);
    const uint32_t off = (uint32_t)(addr & 3u);
    const uint32_t *src = reinterpret_cast<const uint32_t *>(addr - off);
    const int nd = (n + (int)off + 3) >> 2;
    uint64_t acc = terr_nz_nibble(src[0]) >> off;
    int fill = 4 - (int)off;
    for (int i = 1; i < nd; ++i) {                              // (fill <= 63: n <= 64)
        acc |= (uint64_t)terr_nz_nibble(src[i]) << fill;
        fill += 4;
    }
    return n >= 64 ? acc : acc & (((uint64_t)1 << n) - 1u);
}

// the cell one step from (x, y) in direction d (0 up, 1 right, 2 down, 3 left), or -1 off the board
__device__ __forceinline__ int terr_next(const int N, const int x, const int y, const int d)
{
    const int nx = x + ((d & 3) == 1) - ((d & 3) == 3), ny = y + ((d & 3) == 2) - ((d & 3) == 0);
    return ((unsigned)nx < (unsigned)N && (unsigned)ny < (unsigned)N) ? ny * N + nx : -1;
}

// direction offsets of the candidates 0 forward, 1 right, 2 left
__device__ __forceinline__ int terr_turn(const int a) { return a == 0 ? 0 : a == 1 ? 1 : 3; }

struct TerrState {
    int N, NN;
    uint32_t inv_n;            // floor(2^32 / N) + 1: y = umulhi(h, inv_n) is exact for h < N*N <= 2^15
    int64_t B;
    const int8_t *board;
    const int16_t *heads;
    const int8_t *dirs, *deaths;
};

// The first cells of player p in position b, one call of `f(cell)` per cell that is on the board (free or not): the three
// actions, or only `forced` (0..2) when forced >= 0.  Dead players have none.
template <typename F>
__device__ __forceinline__ void terr_first_cells(const TerrState &s, const int64_t b, const int p, const int forced, F f)
{
    const int64_t pb = (int64_t)p * s.B + b;
    if (s.deaths[pb] != 0) return;
    const int h = min(max((int)s.heads[pb], 0), s.NN - 1);      // (a broken state: wrong results, no wild access)
    const int y = (int)__umulhi((uint32_t)h, s.inv_n), x = h - y * s.N;
    const int d = s.dirs[pb] & 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (forced >= 0 && forced != a) continue;
        const int c = terr_next(s.N, x, y, d + terr_turn(a));
        if (c >= 0) f(c);
    }
}

// is the forced first cell of `seat` off the board or occupied?
__device__ __forceinline__ bool terr_fatal(const TerrState &s, const int64_t b, const int seat, const int forced)
{
    bool ok = false;
    terr_first_cells(s, b, seat, forced, [&](const int c) { ok = s.board[b * s.NN + c] == 0; });
    return !ok;
}

// the agent's score of one candidate: own area minus the best other live player's; a fatal candidate below every other
constexpr int kTerrFatalScore = -(1 << 30);

template <int P>
__device__ __forceinline__ int terr_score(const TerrState &s, const int64_t b, const int p, const int (&area)[P], const bool fatal)
{
    if (fatal) return kTerrFatalScore;
    int best = 0;                                               // (areas are >= 0: "no other live player" scores area[p])
#pragma unroll
    for (int q = 0; q < P; ++q)
        if (q != p && s.deaths[(int64_t)q * s.B + b] == 0) best = max(best, area[q]);
    return area[p] - best;
}

// the agent's action for player p of game b from the three scores: the crl_tron_step encoding
__device__ __forceinline__ int terr_decide(const uint32_t gid, const uint32_t c, const int p, const uint32_t k0, const uint32_t k1,
                                           const uint64_t thr, const int s0, const int s1, const int s2)
{
    const philox_out w = philox4x32_10(gid, c, (uint32_t)p, CRL_TAG_TRON_TERRITORY, k0, k1);
    int a = s1 > s0 ? 1 : 0;
    a = s2 > (a ? s1 : s0) ? 2 : a;                             // ties: the lowest index
    if ((uint64_t)w.w[0] < thr) a = (int)__umulhi(w.w[1], 3u);
    return a == 2 ? -1 : a;
}

// the k-th set bit of mask
__device__ __forceinline__ int terr_kth_bit(uint32_t mask, int k)
{
    while (k-- > 0) mask &= mask - 1u;
    return (int)__builtin_ctz(mask);
}

// ------------------------------------------------------------------------------------------------ boards up to 64x64
template <int CTRL>
__device__ __forceinline__ uint32_t terr_dpp(const uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);   // (no source lane: 0)
}
template <int CTRL>
__device__ __forceinline__ uint64_t terr_dpp(const uint64_t v)
{
    return (uint64_t)terr_dpp<CTRL>((uint32_t)v) | ((uint64_t)terr_dpp<CTRL>((uint32_t)(v >> 32)) << 32);
}
constexpr int kDppWaveShl1 = 0x130;   // lane i reads lane i + 1
constexpr int kDppWaveShr1 = 0x138;   // lane i reads lane i - 1

__device__ __forceinline__ int terr_popc(const uint32_t v) { return __popc(v); }
__device__ __forceinline__ int terr_popc(const uint64_t v) { return __popcll(v); }

// where a lane sits: instance `inst` of the wave's floor(64 / N), board row `r`
struct TerrLane {
    uint32_t lane, inst, r, last;      // last: the lane of the instance's last row
    bool in_group;
};

__device__ __forceinline__ TerrLane terr_lane(const int N)
{
    TerrLane t;
    t.lane = threadIdx.x & 63u;
    t.inst = t.lane / (uint32_t)N;
    t.r = t.lane - t.inst * (uint32_t)N;
    t.in_group = t.inst < 64u / (uint32_t)N;
    t.last = t.inst * (uint32_t)N + (uint32_t)N - 1u;
    return t;
}

// Row t.r of instance (position b; `seat` forced onto candidate `forced`, or forced < 0: nobody forced): the free cells and
// every player's first cells in this row.
template <int P, typename W>
__device__ __forceinline__ void terr_load_row(const TerrState &s, const TerrLane &t, const int64_t b, const int seat,
                                              const int forced, W &free, W (&nw)[P])
{
    const int N = s.N;
    const W rowmask = (W)(N >= (int)(8 * sizeof(W)) ? ~(W)0 : (((W)1 << N) - 1u));
    free = (W)~terr_occ_run(s.board + b * s.NN + (int64_t)t.r * N, N) & rowmask;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        W bits = 0;
        terr_first_cells(s, b, p, p == seat ? forced : -1, [&](const int c) {
            const int cy = (int)__umulhi((uint32_t)c, s.inv_n);
            if (cy == (int)t.r) bits |= (W)1 << (c - cy * N);
        });
        nw[p] = bits & free;
    }
}

// The flood of every instance of the wave; all 64 lanes take part (lanes outside an instance hold zeros).  On return
// area[p] holds this row's share.
template <int P, typename W>
__device__ __forceinline__ void terr_flood_rows(const int NN, const TerrLane &t, W free, W (&nw)[P], int (&area)[P])
{
    const W up_ok = (t.in_group && t.r > 0u) ? ~(W)0 : (W)0;            // takes from lane - 1: not the first row
    const W dn_ok = (t.in_group && t.lane < t.last) ? ~(W)0 : (W)0;    // takes from lane + 1: not the last row
#pragma unroll
    for (int p = 0; p < P; ++p) area[p] = 0;
    for (int lvl = 0; lvl <= NN; ++lvl) {                        // (hard bound: a level with a new bit claims a cell)
        W once = 0, twice = 0;
#pragma unroll
        for (int p = 0; p < P; ++p) { twice |= once & nw[p]; once |= nw[p]; }
#pragma unroll
        for (int p = 0; p < P; ++p) area[p] += terr_popc((W)(nw[p] & ~twice));
        free &= ~once;
        if (__ballot(once != 0) == 0ull) break;
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const W f = nw[p];
            nw[p] = ((W)(f << 1) | (W)(f >> 1) | (terr_dpp<kDppWaveShr1>(f) & up_ok) | (terr_dpp<kDppWaveShl1>(f) & dn_ok)) & free;
        }
    }
}

// sums area[] over the lanes of each instance into the instance's first lane (two 16-bit sums per shuffled word:
// an area is at most 64 * 64)
template <int P>
__device__ __forceinline__ void terr_reduce_rows(const TerrLane &t, int (&area)[P])
{
    constexpr int H = (P + 1) / 2;
    uint32_t v[H];
#pragma unroll
    for (int j = 0; j < H; ++j) v[j] = 0u;
#pragma unroll
    for (int p = 0; p < P; ++p) v[p >> 1] |= (uint32_t)area[p] << ((p & 1) * 16);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const bool take = t.lane + (uint32_t)off <= t.last;
#pragma unroll
        for (int j = 0; j < H; ++j) {
            const uint32_t o = (uint32_t)__shfl_down((int)v[j], off);
            v[j] += take ? o : 0u;
        }
    }
#pragma unroll
    for (int p = 0; p < P; ++p) area[p] = (int)((v[p >> 1] >> ((p & 1) * 16)) & 0xffffu);
}

// crl_tron_territory, boards up to 64x64: instance i = b * A + a, floor(64 / N) consecutive instances per wave
template <int P, typename W>
__global__ void __launch_bounds__(256)
tron_territory_rows_kernel(const TerrState s, const int8_t *__restrict__ seat, const int32_t *__restrict__ cand, const int A,
                           const uint64_t n_inst, int32_t *__restrict__ area_out, uint8_t *__restrict__ info)
{
    const TerrLane t = terr_lane(s.N);
    const uint32_t G = 64u / (uint32_t)s.N;
    const uint64_t stride = (uint64_t)gridDim.x * (blockDim.x >> 6) * G;
    for (uint64_t i0 = ((uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * G; i0 < n_inst; i0 += stride) {
        const uint64_t i = i0 + t.inst;
        const bool have = t.in_group && i < n_inst;
        W free = 0, nw[P];
#pragma unroll
        for (int p = 0; p < P; ++p) nw[p] = 0;
        int64_t b = 0;
        int sp = -1, first = -1;
        bool eval = have;
        if (have) {
            b = (int64_t)(i / (uint32_t)A);
            if (cand != nullptr) {
                sp = seat ? (int)seat[b] : 0;
                first = cand[i];
                eval = (unsigned)sp < (unsigned)P && (unsigned)first <= 2u && s.deaths[(int64_t)sp * s.B + b] == 0;
            }
            if (eval) terr_load_row<P, W>(s, t, b, sp, first, free, nw);
        }
        int area[P];
        terr_flood_rows<P, W>(s.NN, t, free, nw, area);
        terr_reduce_rows<P>(t, area);
        if (have && t.r == 0u) {                                // (a skipped instance flooded nothing: zeros)
#pragma unroll
            for (int p = 0; p < P; ++p) area_out[i * P + p] = area[p];
            info[i] = (uint8_t)(eval ? (1u | ((first >= 0 && terr_fatal(s, b, sp, first)) ? 2u : 0u)) : 0u);
        }
    }
}

// crl_tron_sample_territory, boards up to 64x64: one wave per game (every decision of a game reads its step counter in
// the wave that advances it), the game's (masked player, candidate) pairs in chunks of floor(64 / N) instances; the scores
// cross from the instances' first lanes to the deciding lanes through a wave-private LDS row.
template <int P, typename W>
__global__ void __launch_bounds__(256)
tron_sample_territory_rows_kernel(const TerrState s, const uint32_t seed_lo, const uint32_t seed_hi, const uint64_t first_env_id,
                                  uint32_t *__restrict__ tcount, const int advance, const uint64_t thr, const uint32_t pmask,
                                  int8_t *__restrict__ actions)
{
    __shared__ int s_score[4][P * 3];
    int *score = s_score[threadIdx.x >> 6];
    const TerrLane t = terr_lane(s.N);
    const uint32_t G = 64u / (uint32_t)s.N;
    const int nm = __popc(pmask), n_pairs = nm * 3;
    const int64_t stride = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t b = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); b < s.B; b += stride) {
        const uint32_t c = tcount[b];
        for (int k0 = 0; k0 < n_pairs; k0 += (int)G) {
            const int k = k0 + (int)t.inst;
            const bool have = t.in_group && k < n_pairs;
            const int p = have ? terr_kth_bit(pmask, k / 3) : 0, a = k % 3;
            const bool eval = have && s.deaths[(int64_t)p * s.B + b] == 0;
            W free = 0, nw[P];
#pragma unroll
            for (int q = 0; q < P; ++q) nw[q] = 0;
            if (eval) terr_load_row<P, W>(s, t, b, p, a, free, nw);
            int area[P];
            terr_flood_rows<P, W>(s.NN, t, free, nw, area);
            terr_reduce_rows<P>(t, area);
            if (eval && t.r == 0u) score[k] = terr_score<P>(s, b, p, area, terr_fatal(s, b, p, a));
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the scores, before the deciding lanes read them
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if ((int)t.lane < nm) {
            const int p = terr_kth_bit(pmask, (int)t.lane);
            const int64_t pb = (int64_t)p * s.B + b;
            int code = 0;                                       // dead players' rows: 0
            if (s.deaths[pb] == 0)
                code = terr_decide((uint32_t)(first_env_id + (uint64_t)b), c, p, seed_lo, seed_hi, thr, score[3 * t.lane],
                                   score[3 * t.lane + 1], score[3 * t.lane + 2]);
            actions[pb] = (int8_t)code;
        }
        if (advance && t.lane == 0u) tcount[b] = c + 1u;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the next game's scores stay behind these reads
        __builtin_amdgcn_wave_barrier();
    }
}

// ------------------------------------------------------------------------------------------------ boards 65..181 wide
// One workgroup per instance.  LDS: word j of row y of bitboard k at (k * N + y) * RW + j, RW = ceil(N / 32); bitboard 0
// is `free`, 1 + p the frontier of player p.  A thread owns the words w = tid + 256 m, m < kTerrWordsPerThread.
constexpr int kTerrLdsThreads = 256;
constexpr int kTerrWordsPerThread = 5;        // ceil(181 * 6 / 256)

struct TerrWide {
    int RW, nwords;
};

// builds the instance in LDS; returns with a barrier behind it
template <int P>
__device__ __forceinline__ void terr_wide_load(const TerrState &s, const TerrWide &g, uint32_t *lds, const int64_t b,
                                               const int seat, const int forced, const bool eval)
{
    const int N = s.N;
    for (int w = threadIdx.x; w < g.nwords; w += kTerrLdsThreads) {
        const int y = w / g.RW, j = w - y * g.RW;
        const int n = min(32, N - 32 * j);
        lds[w] = eval ? ~(uint32_t)terr_occ_run(s.board + b * s.NN + (int64_t)y * N + 32 * j, n) & (n >= 32 ? ~0u : (1u << n) - 1u) : 0u;
#pragma unroll
        for (int p = 0; p < P; ++p) lds[(1 + p) * g.nwords + w] = 0u;
    }
    __syncthreads();
    if ((int)threadIdx.x < P && eval) {                         // one thread per frontier board: no two write a word
        const int p = (int)threadIdx.x;
        terr_first_cells(s, b, p, p == seat ? forced : -1, [&](const int c) {
            const int cy = (int)__umulhi((uint32_t)c, s.inv_n), cx = c - cy * N;
            const int w = cy * g.RW + (cx >> 5);
            lds[(1 + p) * g.nwords + w] |= (1u << (cx & 31)) & lds[w];
        });
    }
    __syncthreads();
}

// floods the instance in LDS; area[p] of thread 0 holds the totals on return (summed through s_area)
template <int P>
__device__ __forceinline__ void terr_wide_flood(const TerrState &s, const TerrWide &g, uint32_t *lds, int *s_area, int (&area)[P])
{
    const int N = s.N;
#pragma unroll
    for (int p = 0; p < P; ++p) area[p] = 0;
    if ((int)threadIdx.x < P) s_area[threadIdx.x] = 0;
    uint32_t e[P][kTerrWordsPerThread];
    for (int lvl = 0; lvl <= s.NN; ++lvl) {                      // (hard bound: a level with a new bit claims a cell)
        // ---- read: the new cells of every player in the words this thread owns (level 0: the first cells as they stand)
#pragma unroll
        for (int m = 0; m < kTerrWordsPerThread; ++m) {
            const int w = (int)threadIdx.x + kTerrLdsThreads * m;
            const bool own = w < g.nwords;
            const int y = own ? w / g.RW : 0, j = w - y * g.RW;
            const uint32_t free = own ? lds[w] : 0u;
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const uint32_t *f = lds + (1 + p) * g.nwords;
                uint32_t x = 0u;
                if (own) {
                    const uint32_t c = f[w];
                    if (lvl == 0) x = c;
                    else {
                        x = (c << 1) | (c >> 1);
                        if (j > 0) x |= f[w - 1] >> 31;
                        if (j + 1 < g.RW) x |= f[w + 1] << 31;
                        if (y > 0) x |= f[w - g.RW];
                        if (y + 1 < N) x |= f[w + g.RW];
                        x &= free;
                    }
                }
                e[p][m] = x;
            }
        }
        __syncthreads();
        // ---- write: claim, count, retire the claimed cells
        uint32_t any = 0u;
#pragma unroll
        for (int m = 0; m < kTerrWordsPerThread; ++m) {
            const int w = (int)threadIdx.x + kTerrLdsThreads * m;
            if (w >= g.nwords) continue;
            uint32_t once = 0u, twice = 0u;
#pragma unroll
            for (int p = 0; p < P; ++p) { twice |= once & e[p][m]; once |= e[p][m]; }
#pragma unroll
            for (int p = 0; p < P; ++p) {
                area[p] += __popc(e[p][m] & ~twice);
                lds[(1 + p) * g.nwords + w] = e[p][m];
            }
            lds[w] &= ~once;
            any |= once;
        }
        if (__syncthreads_or(any != 0u) == 0) break;
    }
#pragma unroll
    for (int p = 0; p < P; ++p)
        if (area[p]) atomicAdd(&s_area[p], area[p]);
    __syncthreads();
#pragma unroll
    for (int p = 0; p < P; ++p) area[p] = s_area[p];
    __syncthreads();                                            // (s_area is zeroed again by the next flood)
}

template <int P>
__global__ void __launch_bounds__(kTerrLdsThreads)
tron_territory_wide_kernel(const TerrState s, const TerrWide g, const int8_t *__restrict__ seat, const int32_t *__restrict__ cand,
                           const int A, const uint64_t n_inst, int32_t *__restrict__ area_out, uint8_t *__restrict__ info)
{
    extern __shared__ uint32_t terr_lds[];
    __shared__ int s_area[P];
    for (uint64_t i = blockIdx.x; i < n_inst; i += gridDim.x) {
        const int64_t b = (int64_t)(i / (uint32_t)A);
        int sp = -1, first = -1;
        bool eval = true;
        if (cand != nullptr) {
            sp = seat ? (int)seat[b] : 0;
            first = cand[i];
            eval = (unsigned)sp < (unsigned)P && (unsigned)first <= 2u && s.deaths[(int64_t)sp * s.B + b] == 0;
        }
        terr_wide_load<P>(s, g, terr_lds, b, sp, first, eval);
        int area[P];
        terr_wide_flood<P>(s, g, terr_lds, s_area, area);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int p = 0; p < P; ++p) area_out[i * P + p] = eval ? area[p] : 0;
            info[i] = (uint8_t)(eval ? (1u | ((first >= 0 && terr_fatal(s, b, sp, first)) ? 2u : 0u)) : 0u);
        }
    }
}

template <int P>
__global__ void __launch_bounds__(kTerrLdsThreads)
tron_sample_territory_wide_kernel(const TerrState s, const TerrWide g, const uint32_t seed_lo, const uint32_t seed_hi,
                                  const uint64_t first_env_id, uint32_t *__restrict__ tcount, const int advance,
                                  const uint64_t thr, const uint32_t pmask, int8_t *__restrict__ actions)
{
    extern __shared__ uint32_t terr_lds[];
    __shared__ int s_area[P];
    __shared__ int s_score[P * 3];
    const int nm = __popc(pmask);
    for (int64_t b = blockIdx.x; b < s.B; b += gridDim.x) {
        const uint32_t c = tcount[b];
        for (int k = 0; k < nm * 3; ++k) {
            const int p = terr_kth_bit(pmask, k / 3), a = k % 3;
            if (s.deaths[(int64_t)p * s.B + b] != 0) continue;  // (uniform over the workgroup)
            terr_wide_load<P>(s, g, terr_lds, b, p, a, true);
            int area[P];
            terr_wide_flood<P>(s, g, terr_lds, s_area, area);
            if (threadIdx.x == 0) s_score[k] = terr_score<P>(s, b, p, area, terr_fatal(s, b, p, a));
        }
        __syncthreads();
        if ((int)threadIdx.x < nm) {
            const int p = terr_kth_bit(pmask, (int)threadIdx.x);
            const int64_t pb = (int64_t)p * s.B + b;
            int code = 0;                                       // dead players' rows: 0
            if (s.deaths[pb] == 0)
                code = terr_decide((uint32_t)(first_env_id + (uint64_t)b), c, p, seed_lo, seed_hi, thr, s_score[3 * threadIdx.x],
                                   s_score[3 * threadIdx.x + 1], s_score[3 * threadIdx.x + 2]);
            actions[pb] = (int8_t)code;
        }
        if (advance && threadIdx.x == 0) tcount[b] = c + 1u;
        __syncthreads();
    }
}

TerrState terr_state(const crl_tron_cfg &cfg, const int64_t B, const int8_t *board, const int16_t *heads, const int8_t *dirs,
                     const int8_t *deaths)
{
    TerrState s;
    s.N = cfg.N;
    s.NN = cfg.N * cfg.N;
    s.inv_n = (uint32_t)(((uint64_t)1 << 32) / (uint64_t)cfg.N) + 1u;
    s.B = B;
    s.board = board;
    s.heads = heads;
    s.dirs = dirs;
    s.deaths = deaths;
    return s;
}

TerrWide terr_wide(const crl_tron_cfg &cfg)
{
    TerrWide g;
    g.RW = (cfg.N + 31) >> 5;
    g.nwords = cfg.N * g.RW;
    return g;
}

constexpr unsigned kTerrMaxBlocks = 1u << 20;   // grid-stride loops beyond

} // namespace

int crl_tron_territory(const crl_ctx *ctx, int64_t B, const int8_t *board, const int16_t *heads, const int8_t *dirs,
                       const int8_t *deaths, const int8_t *seat, const int32_t *cand, int A, int32_t *area, uint8_t *info,
                       void *stream)
{
    TRON_CTX_CHECK("crl_tron_territory");
    CRL_REQUIRE(board && heads && dirs && deaths, "crl_tron_territory: NULL state pointer");
    CRL_REQUIRE(area && info, "crl_tron_territory: NULL output pointer");
    CRL_REQUIRE(A >= 1 && A <= 16, "crl_tron_territory: A=%d out of range 1..16", A);
    CRL_REQUIRE(cand != nullptr || A == 1, "crl_tron_territory: A=%d with cand == NULL (must be 1)", A);
    const crl_tron_cfg &cfg = ctx->tron;
    const TerrState s = terr_state(cfg, B, board, heads, dirs, deaths);
    const uint64_t n_inst = (uint64_t)B * (uint64_t)A;
    hipStream_t st = (hipStream_t)stream;
    if (cfg.N <= 64) {
        const uint64_t per_block = 4u * (64u / (unsigned)cfg.N);
        const uint64_t want = (n_inst + per_block - 1) / per_block;
        const unsigned blocks = (unsigned)(want < kTerrMaxBlocks ? want : kTerrMaxBlocks);
        TRON_DISPATCH_P(cfg.P, {
            if (cfg.N <= 32)
                hipLaunchKernelGGL((tron_territory_rows_kernel<PP, uint32_t>), dim3(blocks), dim3(256), 0, st, s, seat, cand, A,
                                   n_inst, area, info);
            else
                hipLaunchKernelGGL((tron_territory_rows_kernel<PP, uint64_t>), dim3(blocks), dim3(256), 0, st, s, seat, cand, A,
                                   n_inst, area, info);
        });
    } else {
        const TerrWide g = terr_wide(cfg);
        const unsigned blocks = (unsigned)(n_inst < kTerrMaxBlocks ? n_inst : kTerrMaxBlocks);
        const size_t lds = (size_t)(1 + cfg.P) * g.nwords * sizeof(uint32_t);       // at most 9 * 1,086 words: 39 KB
        TRON_DISPATCH_P(cfg.P, {
            hipLaunchKernelGGL((tron_territory_wide_kernel<PP>), dim3(blocks), dim3(kTerrLdsThreads), lds, st, s, g, seat, cand, A,
                               n_inst, area, info);
        });
    }
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

int crl_tron_sample_territory(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, uint32_t *tcount, int advance,
                              double noise, uint32_t player_mask, const int8_t *board, const int16_t *heads, const int8_t *dirs,
                              const int8_t *deaths, int8_t *actions, void *stream)
{
    TRON_CTX_CHECK("crl_tron_sample_territory");
    CRL_REQUIRE(tcount && actions, "crl_tron_sample_territory: NULL tcount / actions pointer");
    CRL_REQUIRE(board && heads && dirs && deaths, "crl_tron_sample_territory: NULL state pointer");
    CRL_REQUIRE(noise >= 0.0 && noise <= 1.0, "crl_tron_sample_territory: noise=%g not in [0, 1]", noise);
    const crl_tron_cfg &cfg = ctx->tron;
    CRL_REQUIRE((player_mask >> cfg.P) == 0u, "crl_tron_sample_territory: player_mask 0x%x names players beyond P=%d", player_mask, cfg.P);
    const TerrState s = terr_state(cfg, B, board, heads, dirs, deaths);
    const uint64_t thr = crl_noise_threshold(noise);
    hipStream_t st = (hipStream_t)stream;
    if (cfg.N <= 64) {
        const uint64_t want = ((uint64_t)B + 3u) / 4u;
        const unsigned blocks = (unsigned)(want < kTerrMaxBlocks ? want : kTerrMaxBlocks);
        TRON_DISPATCH_P(cfg.P, {
            if (cfg.N <= 32)
                hipLaunchKernelGGL((tron_sample_territory_rows_kernel<PP, uint32_t>), dim3(blocks), dim3(256), 0, st, s, (uint32_t)seed,
                                   (uint32_t)(seed >> 32), first_env_id, tcount, advance, thr, player_mask, actions);
            else
                hipLaunchKernelGGL((tron_sample_territory_rows_kernel<PP, uint64_t>), dim3(blocks), dim3(256), 0, st, s, (uint32_t)seed,
                                   (uint32_t)(seed >> 32), first_env_id, tcount, advance, thr, player_mask, actions);
        });
    } else {
        const TerrWide g = terr_wide(cfg);
        const unsigned blocks = (unsigned)((uint64_t)B < kTerrMaxBlocks ? (uint64_t)B : kTerrMaxBlocks);
        const size_t lds = (size_t)(1 + cfg.P) * g.nwords * sizeof(uint32_t);
        TRON_DISPATCH_P(cfg.P, {
            hipLaunchKernelGGL((tron_sample_territory_wide_kernel<PP>), dim3(blocks), dim3(kTerrLdsThreads), lds, st, s, g,
                               (uint32_t)seed, (uint32_t)(seed >> 32), first_env_id, tcount, advance, thr, player_mask, actions);
        });
    }
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}
