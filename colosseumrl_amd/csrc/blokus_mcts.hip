// blokus_mcts.hip -- batched tree search with progressive widening for Blokus (crl_blokus_mcts; the contract is in
// include/colosseum_hip.h), gfx950, wave64.  The rules, the tables and the per-wave working set are blokus.hip's, taken
// in by including that file up to its kernels; the tree and the search are blokus_mcts_search.hpp's, which the seated
// search agent (blokus_mcts_agent.hip) runs too.  The search is a translation unit of its own so that blokus.hip's kernels
// stay what they are (see the note in blokus.hip).  What is left here is what this entry alone has: the candidate root's
// pre-pass (the playable columns, and the stores of a row that is skipped), the root row's stores and the entry's checks.
#define BLK_DEVICE_ONLY
#include "blokus.hip"
#include "blokus_mcts_search.hpp"

namespace {

// 4 waves per SIMD: the trees' LDS admits no more workgroups per CU than that anyway (S = 128: 18.6 + 17.5 KB of 160)
template <bool GROUP>
__global__ void __launch_bounds__(256, 4)
blokus_mcts_kernel(const BlkTables *__restrict__ tables, const int64_t B, const uint32_t seed_lo, const uint32_t seed_hi,
                   const uint64_t first_env_id, const uint32_t *__restrict__ occ, const uint32_t *__restrict__ inv_g,
                   const int32_t *__restrict__ score_g, const int32_t *__restrict__ round_g,
                   const int32_t *__restrict__ to_move_g, const uint32_t *__restrict__ tcount,
                   const int32_t *__restrict__ cand, const int A, const int W, const int S, const int R, const uint32_t cexp,
                   const uint32_t tree_words, const int trees, int32_t *__restrict__ ids_g, uint32_t *__restrict__ visits_g,
                   uint32_t *__restrict__ value_g, uint32_t *__restrict__ nodes_g, int32_t *__restrict__ best_g)
{
    BLK_WAVE_SETUP();
    extern __shared__ __attribute__((aligned(16))) uint32_t blk_mcts_lds[];
    if (!GROUP && wave_ >= trees) return;                       // (behind the set-up's barrier, the only one of this mapping)
    const int64_t b = GROUP ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * trees + wave_;
    if (b >= B) return;                                          // (a whole workgroup when GROUP)
    const bool writer = !GROUP || wave_ == 0;
    const BlkTree tr = blk_tree_layout<GROUP>(blk_mcts_lds, wave_, tree_words, S);
    const BlkSearchArgs sa = {W, S, R, cexp, seed_lo, seed_hi};
    const uint32_t piece_cells = lane < 24 ? T.ncell[lane] : 0u;
    const BlkOwners owners = blk_shape_owners(T, lane);
    const uint32_t root_a = occ[b * 4 * BN + lane], root_b = lane < 4 * BN - 64 ? occ[b * 4 * BN + 64 + lane] : 0u;
    const uint32_t root_vinv = inv_g[b * 4 + (lane & 3)];
    const int root_vscore = score_g[b * 4 + (lane & 3)];
    const int round0 = __builtin_amdgcn_readfirstlane(round_g[b]), pl0 = __builtin_amdgcn_readfirstlane(to_move_g[b]) & 3;
    const uint32_t tc0 = tcount ? (uint32_t)__builtin_amdgcn_readfirstlane((int)tcount[b]) : 0u;
    const uint32_t g = (uint32_t)(first_env_id + (uint64_t)b);
    const int K = cand != nullptr ? A : W;
    // ---- a candidate root: the playable columns (legal for the mover, and no repeat of an earlier playable one)
    unsigned long long playable = 0ull;
    const int cand_v = (cand != nullptr && lane < A) ? cand[b * A + lane] : -3;
    if (cand != nullptr) {
        uint32_t *flat = &L.occ[0][0];                           // the board's 80 row words: lane i holds words i and 64 + i
        flat[lane] = root_a;
        if (lane < 4 * BN - 64) flat[64 + lane] = root_b;
        wave_sync();
        blk_prep(L, lane, round0);
        const uint32_t ip = (uint32_t)__builtin_amdgcn_readlane((int)root_vinv, pl0);
        for (int a = 0; a < A; ++a) {
            const int id = __builtin_amdgcn_readlane(cand_v, a);
            if (id < 0 || id >= ACTION_IDS) continue;
            if (!blk_move_legal<false>(T, L, pl0, ip, blk_decode(id), lane)) continue;
            if (__ballot(cand_v == id && lane < a) & playable) continue;
            playable |= 1ull << a;
        }
        if (playable == 0ull) {                                  // the row is skipped
            if (writer) {
                if (lane < K) { ids_g[b * K + lane] = -2; visits_g[b * K + lane] = 0u; value_g[b * K + lane] = 0u; }
                if (lane == 0) { nodes_g[b] = 0u; best_g[b] = -2; }
            }
            return;
        }
    }
    (void)blk_mcts_search<GROUP>(T, L, lane, wave_, tr, root_a, root_b, root_vinv, root_vscore, round0, pl0, tc0, g, sa, piece_cells,
                                 owners, cand != nullptr, cand_v, playable,
                                 [&](const int cid, const uint32_t vis, const uint32_t val, const int nn, const int best_id) {
        if (lane < K) { ids_g[b * K + lane] = cid; visits_g[b * K + lane] = vis; value_g[b * K + lane] = val; }
        if (lane == 0) { nodes_g[b] = (uint32_t)nn; best_g[b] = best_id; }
    });
}

} // namespace

int crl_blokus_mcts_bounds(unsigned int *out4)
{
    CRL_BOUNDS_READBACK(out4);
    return CRL_OK;
}

extern "C" {

int crl_blokus_mcts_max_simulations(const crl_ctx *ctx)
{
    CRL_REQUIRE(ctx != nullptr && ctx->game == CRL_GAME_BLOKUS && ctx->blokus, "crl_blokus_mcts_max_simulations: ctx is not a blokus context");
    return BLK_MCTS_MAX_S;
}

int crl_blokus_mcts(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id,
                    const uint32_t *occ, const uint32_t *inv, const int32_t *score, const int32_t *round,
                    const int32_t *to_move, const uint32_t *tcount,
                    const int32_t *cand, int A, int W, int S, int R, uint32_t cexp,
                    int32_t *ids, uint32_t *visits, uint32_t *value, uint32_t *nodes, int32_t *best,
                    uint32_t flags, void *stream)
{
    // (the pointer and argument checks come before the context's: they need no device)
    CRL_REQUIRE(occ && inv && score && round && to_move, "crl_blokus_mcts: NULL state pointer");
    CRL_REQUIRE(ids && visits && value && nodes && best, "crl_blokus_mcts: NULL output pointer");
    BLK_MCTS_BATCH_CHECK("crl_blokus_mcts");
    CRL_REQUIRE(cand == nullptr || (A >= 1 && A <= 64), "crl_blokus_mcts: A=%d out of range 1..64", A);
    CRL_REQUIRE(cand != nullptr || A == 1, "crl_blokus_mcts: A=%d with cand == NULL (must be 1)", A);
    BLK_MCTS_SEARCH_CHECK("crl_blokus_mcts");
    CRL_REQUIRE(flags == 0, "crl_blokus_mcts: unknown flags 0x%x", flags);
    CRL_REQUIRE(ctx != nullptr && ctx->game == CRL_GAME_BLOKUS && ctx->blokus, "crl_blokus_mcts: ctx is not a blokus context");
    blk_mcts_dispatch(B, S, R, [&](auto group, unsigned grid, uint32_t lds_bytes, uint32_t tree_words, int trees) {
        hipLaunchKernelGGL(blokus_mcts_kernel<decltype(group)::value>, dim3(grid), dim3(256), lds_bytes, (hipStream_t)stream,
                           (const BlkTables *)ctx->blokus, B, (uint32_t)seed, (uint32_t)(seed >> 32), first_env_id,
                           occ, inv, score, round, to_move, tcount, cand, A, W, S, R, cexp, tree_words, trees,
                           ids, visits, value, nodes, best);
    });
    CRL_LAUNCH_CHECK();
    return CRL_OK;
}

} // extern "C"
