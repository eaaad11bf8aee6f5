// tron_lane_table.hpp -- what a lane of tron_rollout_quad_kernel needs that depends on the context alone (board width, players,
// start layout) and on the lane's place in its workgroup, never on the batch or on a launch: built once per context on the
// host (crl_tron_create), uploaded once per device, read by every launch with three 16-byte loads per lane.  Plain C++, no
// HIP: the library, a host test (crl_tron_lane_table) and a stand-alone program can all call the builder.
//
// Geometry (tron.hip, the byte-slab lane-per-player kernel): 256 threads = 64 games x 4 seats, thread t plays seat t & 3 of
// the game in slab t >> 2; a slab is N + 2 rows of RS = 24 bytes (row 0 and row N + 1 wall, cell (y, x) at (y + 1) * RS + x,
// bytes N..23 of a row wall) plus a junk dword, padded to an odd number of dwords.  Wave w copies the boards of slabs
// 16 w .. 16 w + 15 by rows: lane l takes rows R = l + 64 k (k = 0..4) of the wave's 16 N, row R = N e + r being row r of the
// wave's game e.  Every offset below is a byte offset from the workgroup's first slab, so one table serves every workgroup.
//
// Per thread t, kTronLaneWords = 12 dwords at 12 t:
//   0..4   row k: LDS offset of the row's first cell | LDS offset of its game's junk byte << 16 (0xffffffff: no such row)
//   5      seat start cell (a seat without a player: its junk byte) | my first dword of slab row 1 (the rolling rewrite) << 16
//   6      my junk byte (slab junk + seat) | wall dword 0 << 16
//   7      wall dword 1 | wall dword 2 << 16     (the slab's 12 wall dwords of rows 0 and N + 1, three per seat)
//   8, 9   my two dwords of a freshly rewritten row (dwords seat and seat + 2 of its six: 0xff where the byte is wall)
//   10     seat start direction << 3 | (the seat has a player) << 8
//   11     0
// Behind the 256 threads, at dword kTronLaneLutWord: the 81 action-code bytes of the random agent (+ 3 zero bytes).
#pragma once
#include <cstdint>

constexpr int kTronLaneThreads = 256, kTronLaneWords = 12, kTronLaneRows = 5, kTronLaneRowBytes = 24;
constexpr int kTronLaneLutWord = kTronLaneThreads * kTronLaneWords;
constexpr int kTronLaneLutWords = 21;                            // 81 bytes, rounded up
constexpr int kTronLaneTableWords = kTronLaneLutWord + kTronLaneLutWords + 3;   // a whole number of 16-byte pieces
constexpr int kTronLaneMaxN = 20, kTronLaneMaxP = 4;

// bytes per slab: the junk dword behind N + 2 rows, a whole ODD number of dwords (tron.hip: pad_of)
inline int crl_tron_lane_stride(const int N)
{
    int stride = ((N + 2) * kTronLaneRowBytes + 1 + 3) & ~3;
    if (((stride >> 2) & 1) == 0) stride += 4;
    return stride;
}

// out: kTronLaneTableWords dwords.  2 <= N <= kTronLaneMaxN, 1 <= P <= kTronLaneMaxP, start_heads[p] in [0, N * N)
inline void crl_tron_lane_table_build(const int N, const int P, const int16_t *start_heads, const int8_t *start_dirs, uint32_t *out)
{
    constexpr int RS = kTronLaneRowBytes, kWaveGames = 16;
    const int junk = (N + 2) * RS, stride = crl_tron_lane_stride(N);
    for (int t = 0; t < kTronLaneThreads; ++t) {
        uint32_t *w = out + t * kTronLaneWords;
        const int lane = t & 63, wave = t >> 6, p = t & 3, slot = t >> 2;
        const int mine = slot * stride, slab0 = wave * kWaveGames * stride;
        for (int k = 0; k < kTronLaneRows; ++k) {
            const int R = lane + 64 * k;
            if (R < kWaveGames * N) {
                const int e = R / N, r = R % N;
                const int sb = slab0 + e * stride;
                w[k] = (uint32_t)(sb + (r + 1) * RS) | (uint32_t)(sb + junk) << 16;
            } else {
                w[k] = 0xffffffffu;
            }
        }
        const bool seated = p < P;
        const int my_junk = mine + junk + p;
        const int fh = seated ? start_heads[p] : 0;
        const int fresh_h = seated ? mine + (fh / N + 1) * RS + fh % N : my_junk;
        int wall[3];
        for (int i = 0; i < 3; ++i) {
            const int dw = 3 * p + i;
            wall[i] = mine + (dw < 6 ? 4 * dw : (N + 1) * RS + 4 * (dw - 6));
        }
        w[5] = (uint32_t)fresh_h | (uint32_t)(mine + RS + 4 * p) << 16;
        w[6] = (uint32_t)my_junk | (uint32_t)wall[0] << 16;
        w[7] = (uint32_t)wall[1] | (uint32_t)wall[2] << 16;
        for (int i = 0; i < 2; ++i) {
            const int j = p + 2 * i;
            uint32_t m = 0;
            for (int c = 0; c < 4; ++c) m |= (4 * j + c < N) ? 0u : (0xffu << (8 * c));
            w[8 + i] = m;
        }
        w[10] = (uint32_t)((seated ? start_dirs[p] & 3 : 0) << 3) | (seated ? 1u << 8 : 0u);
        w[11] = 0u;
    }
    // the action table: entry t = four base-3 digits of t, each as a 2-bit code (0, 1, 3), first digit in bits 1:0
    uint32_t *lut = out + kTronLaneLutWord;
    for (int i = 0; i < kTronLaneLutWords + 3; ++i) lut[i] = 0u;
    for (uint32_t t = 0; t < 81u; ++t) {
        const uint32_t a[4] = {t / 27u, (t / 9u) % 3u, (t / 3u) % 3u, t % 3u};
        uint32_t code = 0;
        for (int i = 0; i < 4; ++i) code |= (a[i] + (a[i] >> 1)) << (2 * i);
        lut[t >> 2] |= code << (8 * (t & 3u));
    }
}
