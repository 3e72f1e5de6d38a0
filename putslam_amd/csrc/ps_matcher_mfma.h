// ps_matcher_mfma.h -- kernel 1 of the path on the matrix cores of gfx950.
//
// cv::batchDistance(train, query, K=1) inside BFMatcher's cross-check (reference call site
// src/Matcher/matcherOpenCV.cpp:198-206): for each train row the nearest query row under the 256-bit
// Hamming distance, ties to the lowest query index.
//
// The N x N x 256 popcount sweep is an exact small-integer contraction: with every descriptor bit b
// written as s = 4 - 8b (+4 / -4), sum_k s_q[k] * s_t[k] = 16 * (256 - 2 * hamming).  +-4 are FP4 (e2m1) values, so
// v_mfma_f32_32x32x64_f8f6f4 with FP4 operands (the densest matrix format of CDNA4: K = 64 per 32-cycle
// instruction) computes a 32 x 32 tile of distances in 4 instructions; every partial sum is an integer below
// 2^13, hence exact in the f32 accumulator whatever the internal summation order.  The accumulator is
// initialised with 2^23 + 4127 - (row of the tile), so each entry ends as
//       2^23 + D,   D = 8223 - 32 * hamming - row = 32 * (256 - hamming) + (31 - row)   in [0, 8223]
// Every value (and every partial sum) lies in [2^23, 2^24), where f32 has unit spacing: the mantissa field of
// the result IS the integer D and the bit patterns order like integers.  Within a tile the nearest query, lowest
// row first, is the MAXIMUM pattern: v_max3_i32 over the 16 accumulator registers a lane holds (its column = its
// train descriptor).  Across tiles (ascending query index) a later tile wins only with a strictly smaller
// distance, i.e. when its maximum exceeds the running best with the row field saturated (best | 31): one v_or,
// one compare, two selects per tile.  Query rows beyond the frame start from -1e30 (a negative pattern).
//
// Operand traffic: the previous frame (query side) of every pair is expanded once per call into the
// fragment-major FP4 image  Xq[pair][tile of 32 rows][k-step 0..3][lane 0..63][16 B]  by ps_expand_query_fp4
// (N work, not N^2); every wave expands its own TT train tiles in registers once and keeps them as B operands for
// the whole sweep, and streams the query tiles as A operands: four contiguous 1-KiB loads per tile, one tile ahead,
// straight into registers (the four waves of a work-group read the same tiles within a few hundred cycles: L1 / L2
// hits).  The first form staged the query tiles through LDS (double-buffered, one barrier per tile, shared by the
// four waves): 0.211 ms against 0.186 ms per 499 pairs -- the barrier tied the waves of a work-group together, and
// with one wave of each of two work-groups per SIMD the matrix and the vector phases of all of them coincided
// (that form left the tree in round 4; the A/B is on file in profiles/r02h).
// Any consistent assignment of descriptor bits to (k-step, lane half, element) is valid because both
// operands use the same one: lane (r = lane & 31, h = lane >> 5) holds, for k-step s, the 32 bits of dword
// 2s + h of row r, and fp4_word below -- the one expansion rule of every form and both sides -- puts bit 4 i + j of that
// dword into nibble i of the lane's operand register j.
//
// The integer VALU kernel ps_hamming_nn (ps_match_stage.h) is kept as the tested twin
// (PUTSLAM_HIP_MATCHER=valu / ps_context_set_option("matcher", 0)).
#pragma once

#include "ps_block.h" // kBlock, xcd_remap
#include "ps_device_math.h"

namespace psdev {

// a keys entry no train row has written: both matchers' blocks are all-ones at rest (kernel 2 puts it back)
constexpr uint32_t kNoKey = 0xFFFFFFFFu;

typedef int v4i_t __attribute__((ext_vector_type(4)));
typedef int v8i_t __attribute__((ext_vector_type(8)));
typedef float v16f_t __attribute__((ext_vector_type(16)));

constexpr int kTileRows = 32;            // rows of one MFMA tile
constexpr int kTileU4 = 256;             // uint4 (16 B) pieces of one expanded tile: 4 k-steps x 64 lanes = 4 KiB
constexpr int kWavesPerWG = kBlock / 64; // 4

// The one expansion rule, table-free: descriptor dword w -> its 32 FP4 values in four dwords.  Nibble i of output dword j
// takes descriptor bit 4 i + j as its sign (bit 3 of e2m1); the low three bits are 0b110 = 4.0: 0 -> 0x6 = +4.0,
// 1 -> 0xE = -4.0.  No bit is spread: one shift and one bit-field insert (v_bfi_b32: (mask & a) | (~mask & b)) per output
// dword, 7 vector instructions per descriptor dword (j = 3 needs no shift).  Both operand sides of every form go through
// this function, which is all the contraction needs (see the header).
// (sign / fill: the two constants; a hot loop hands them in from registers, where the compiler then takes ONE three-operand
// instruction per output dword -- v_bfi_b32 or, as it stands, v_and_or_b32; as literals they cost a v_and and a v_or, gfx950's
// three-operand encodings take no literal)
PS_HD constexpr uint32_t fp4_word(uint32_t w, int j, uint32_t sign = 0x88888888u, uint32_t fill = 0x66666666u)
{
    return (sign & (w << (3 - j))) | (~sign & fill);
}
constexpr bool fp4_word_checks(uint32_t w)
{
    for (int j = 0; j < 4; ++j) {
        const uint32_t o = fp4_word(w, j);
        if ((o & 0x77777777u) != 0x66666666u) return false; // magnitude 4.0 in every nibble
        for (int i = 0; i < 8; ++i)
            if (((o >> (4 * i + 3)) & 1u) != ((w >> (4 * i + j)) & 1u)) return false; // sign of nibble i = bit 4 i + j
    }
    return true;
}
constexpr bool fp4_single_bits_check()
{
    for (int b = 0; b < 32; ++b) { // bit b lands in bit 3 of exactly one nibble of exactly one output dword
        int hits = 0;
        for (int j = 0; j < 4; ++j)
            for (int i = 0; i < 8; ++i)
                if ((fp4_word(1u << b, j) >> (4 * i + 3)) & 1u) hits += (4 * i + j == b) ? 1 : 100;
        if (hits != 1 || !fp4_word_checks(1u << b) || !fp4_word_checks(~(1u << b))) return false;
    }
    return true;
}
static_assert(fp4_single_bits_check(), "every descriptor bit is the sign of exactly one nibble");
static_assert(fp4_word_checks(0u) && fp4_word_checks(0xFFFFFFFFu) && fp4_word_checks(0x80000001u) &&
                  fp4_word_checks(0xDEADBEEFu) && fp4_word_checks(0x01234567u) && fp4_word_checks(0xA5A5C3C3u) &&
                  fp4_word_checks(0x0F0F00FFu) && fp4_word_checks(0x13579BDFu),
              "fp4_word: sign of nibble i of dword j = bit 4 i + j, magnitude 0b110");
static_assert(fp4_word(0u, 0) == 0x66666666u && fp4_word(0xFFFFFFFFu, 2) == 0xEEEEEEEEu && fp4_word(0x10u, 0) == 0x000000E0u + 0x66666606u,
              "fp4_word: 0 -> +4.0, 1 -> -4.0");
PS_D v4i_t fp4_from_dword(uint32_t w)
{
    v4i_t r;
    r.x = (int)fp4_word(w, 0);
    r.y = (int)fp4_word(w, 1);
    r.z = (int)fp4_word(w, 2);
    r.w = (int)fp4_word(w, 3);
    return r;
}

// row of the 32 x 32 tile held in accumulator register `reg` by lane half h (C/D layout of every
// 32x32 MFMA of gfx950: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5))
PS_D int tile_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// ------------------------------------------------------------------------------------------
// Query-side expansion: one work-group per (pair, chunk of tiles).  Thread o of a tile writes piece
// o = s * 64 + h * 32 + r (the layout the MFMA kernel reads back linearly), i.e. dword 2s + h of row r.
// Rows beyond the frame's count are written as zeros (0.0 in FP4); the MFMA kernel masks them anyway.
// ------------------------------------------------------------------------------------------
// (fstride in all three kernels: dwords between consecutive frames' descriptor blocks -- cap * 8 for the dense frame set)
__global__ __launch_bounds__(kBlock) void ps_expand_query_fp4(const uint32_t *__restrict__ desc,
                                                              const int32_t *__restrict__ nkpts,
                                                              const int32_t *__restrict__ pairs, int cap, int fstride, int tpf,
                                                              int chunks, uint4 *__restrict__ Xq,
                                                              uint32_t *__restrict__ keysInit)
{
    // grid = chunks x P work-groups in one dimension (no 65535 limit on the number of pairs)
    const int p = (int)(blockIdx.x / (unsigned)chunks), chunk = (int)(blockIdx.x % (unsigned)chunks);
    if (keysInit) // the matcher merges query splits with atomicMin: start every key at "no query" (saves a memset launch)
        for (int t = chunk * kBlock + threadIdx.x; t < cap; t += chunks * kBlock) keysInit[(size_t)p * cap + t] = kNoKey;
    const int fq = pairs[2 * p];
    const int nq = nkpts[fq];
    const uint32_t *__restrict__ q32 = desc + (size_t)fq * fstride;
    uint4 *__restrict__ out = Xq + (size_t)p * tpf * kTileU4;
    const int o = threadIdx.x, s = o >> 6, h = (o >> 5) & 1, r = o & 31;
    for (int tile = chunk; tile < tpf; tile += chunks) {
        const int row = tile * kTileRows + r;
        v4i_t e = {0, 0, 0, 0};
        if (row < nq) e = fp4_from_dword(q32[(size_t)row * 8 + 2 * s + h]);
        out[(size_t)tile * kTileU4 + o] = make_uint4((uint32_t)e.x, (uint32_t)e.y, (uint32_t)e.z, (uint32_t)e.w);
    }
}

PS_D v16f_t mfma_fp4(const v4i_t &a, const v4i_t &b, const v16f_t &c)
{
    // FP4 operands occupy the first 4 of the 8 operand registers (cbsz = blgp = 4 selects e2m1); scale
    // operands 0 with op_sel 0 select the unscaled form (scale 2^0 on both sides)
    const v8i_t a8 = __builtin_shufflevector(a, a, 0, 1, 2, 3, -1, -1, -1, -1);
    const v8i_t b8 = __builtin_shufflevector(b, b, 0, 1, 2, 3, -1, -1, -1, -1);
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, c, 4, 4, 0, 0, 0, 0);
}

// The same instruction in its block-scaled form with the uniform scales 2^9 (A side) and 2^0 (B side): E8M0 bytes 136 and
// 127 in every byte of the scale operands, so that the result does not depend on which byte a lane's block takes.
PS_D v16f_t mfma_fp4s(const v4i_t &a, const v4i_t &b, const v16f_t &c)
{
    const v8i_t a8 = __builtin_shufflevector(a, a, 0, 1, 2, 3, -1, -1, -1, -1);
    const v8i_t b8 = __builtin_shufflevector(b, b, 0, 1, 2, 3, -1, -1, -1, -1);
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, c, 4, 4, 0, (int)0x88888888u, 0, (int)0x7F7F7F7Fu);
}

PS_D int fbits(float f) { return __builtin_bit_cast(int, f); }
PS_D int imax3(int a, int b, int c) { return max(max(a, b), c); }
// maximum of the 16 accumulator entries as integer bit patterns (valid entries are >= +0.0f)
PS_D int max16(const v16f_t &d)
{
    int m = imax3(fbits(d[0]), fbits(d[1]), fbits(d[2]));
    m = imax3(m, fbits(d[3]), fbits(d[4]));
    m = imax3(m, fbits(d[5]), fbits(d[6]));
    m = imax3(m, fbits(d[7]), fbits(d[8]));
    m = imax3(m, fbits(d[9]), fbits(d[10]));
    m = imax3(m, fbits(d[11]), fbits(d[12]));
    m = imax3(m, fbits(d[13]), fbits(d[14]));
    return max(m, fbits(d[15]));
}

constexpr float kMfmaNoRow = -1.0e30f; // accumulator start of a query row beyond the frame: never the maximum
constexpr int kMfmaBias = 8223;        // 32 * 256 + 31
constexpr float kMfmaBase = 8388608.0f; // 2^23: unit spacing up to 2^24

// ------------------------------------------------------------------------------------------
// grid = groups * qsplit * P work-groups in XCD-aware order; a work-group owns 4 * TT train tiles (one
// wave each TT of them) and sweeps the query tiles [T0, T1) of its split.  qsplit > 1 merges with atomicMin
// on the packed key (hamming << 16 | query), the same key kernel 2 reads from ps_hamming_nn.
// ------------------------------------------------------------------------------------------
// Every wave loads its own query tiles straight into registers (the first form staged them through LDS with a barrier
// per tile, shared by the work-group's four waves: 14 % slower, profiles/r02h).
#ifndef PS_MFMA_WAVES
#define PS_MFMA_WAVES 1
#endif
template <int TT>
__global__ __launch_bounds__(kBlock, PS_MFMA_WAVES) void ps_hamming_mfma(const uint32_t *__restrict__ desc,
                                                          const int32_t *__restrict__ nkpts,
                                                          const int32_t *__restrict__ pairs, int cap, int fstride, int tpf,
                                                          int groups, int qsplit, const uint4 *__restrict__ Xq,
                                                          uint32_t *__restrict__ keys)
{
    const unsigned perPair = (unsigned)(groups * qsplit);
    const unsigned L = xcd_remap(blockIdx.x, gridDim.x);
    const int p = (int)(L / perPair);
    const int inner = (int)(L - (unsigned)p * perPair);
    const int g = inner / qsplit, qs = inner - g * qsplit;
    const int fq = pairs[2 * p], ft = pairs[2 * p + 1]; // query = previous frame, train = current
    const int nq = nkpts[fq], nt = nkpts[ft];
    if (g * (kWavesPerWG * TT * kTileRows) >= nt) return; // whole work-group beyond the train rows
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int tile0 = (g * kWavesPerWG + wave) * TT;
    const int nqTiles = (nq + kTileRows - 1) / kTileRows;
    const int T0 = (int)(((long long)nqTiles * qs) / qsplit), T1 = (int)(((long long)nqTiles * (qs + 1)) / qsplit);

    // B operands: this wave's train tiles, expanded in registers (rows beyond nt repeat the last row; never stored)
    const uint32_t *__restrict__ t32 = desc + (size_t)ft * fstride;
    v4i_t B[TT][4];
#pragma unroll
    for (int i = 0; i < TT; ++i) {
        int t = (tile0 + i) * kTileRows + r;
        t = t < nt ? t : nt - 1;
#pragma unroll
        for (int s = 0; s < 4; ++s) B[i][s] = fp4_from_dword(t32[(size_t)t * 8 + 2 * s + h]);
    }
    v16f_t C;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) C[reg] = kMfmaBase + (float)(kMfmaBias - 4096 - tile_row(reg, h));
    int best[TT], bestT[TT];
#pragma unroll
    for (int i = 0; i < TT; ++i) {
        best[i] = 0; // below every valid entry (their patterns are >= 0x4B000000)
        bestT[i] = 0;
    }

    const uint4 *__restrict__ xq = Xq + (size_t)p * tpf * kTileU4;
    // Every wave fetches its own copy of the query tile (4 x 16 B per lane, served by L1 / L2 for the other waves of the
    // work-group) one tile ahead into registers: no LDS staging, no barrier, the waves of a work-group drift apart freely.
    uint4 an[4];
    if (T0 < T1) {
#pragma unroll
        for (int s = 0; s < 4; ++s) an[s] = xq[(size_t)T0 * kTileU4 + s * 64 + lane];
    }
    for (int T = T0; T < T1; ++T) {
        v4i_t A[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            A[s].x = (int)an[s].x; A[s].y = (int)an[s].y; A[s].z = (int)an[s].z; A[s].w = (int)an[s].w;
        }
        if (T + 1 < T1) {
#pragma unroll
            for (int s = 0; s < 4; ++s) an[s] = xq[(size_t)(T + 1) * kTileU4 + s * 64 + lane];
        }
        v16f_t Cin = C;
        if (T * kTileRows + kTileRows > nq) { // last, partial query tile: rows beyond nq can never win
#pragma unroll
            for (int reg = 0; reg < 16; ++reg)
                if (T * kTileRows + tile_row(reg, h) >= nq) Cin[reg] = kMfmaNoRow;
        }
#pragma unroll
        for (int i = 0; i < TT; ++i) {
            v16f_t acc = mfma_fp4(A[0], B[i][0], Cin);
            acc = mfma_fp4(A[1], B[i][1], acc);
            acc = mfma_fp4(A[2], B[i][2], acc);
            acc = mfma_fp4(A[3], B[i][3], acc);
            const int m = max16(acc);
            if (m > (best[i] | 31)) { // strictly smaller distance only: the earlier (lower) query tile keeps a tie
                best[i] = m;
                bestT[i] = T;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < TT; ++i) {
        const int t = (tile0 + i) * kTileRows + r;
        uint32_t key = kNoKey;
        if (best[i] > 0) {
            const int v = kMfmaBias - (best[i] & 0x7FFFFF); // 32 * hamming + row of the tile
            key = ((uint32_t)(v >> 5) << 16) | (uint32_t)(bestT[i] * kTileRows + (v & 31));
        }
        const uint32_t other = (uint32_t)__shfl_xor((int)key, 32, 64); // the other half's 16 rows of every tile
        key = other < key ? other : key;
        if (h == 0 && t < nt) {
            if (qsplit == 1)
                keys[(size_t)p * cap + t] = key;
            else
                atomicMin(&keys[(size_t)p * cap + t], key);
        }
    }
}

// ------------------------------------------------------------------------------------------
// Fused form (default since round 3): no FP4 image in HBM and no expansion launch.  The work-group expands the query
// tiles itself, kFuseChunk tiles at a time, into a double-buffered LDS image in the same fragment-major layout
// (thread o of the group writes piece o of every tile of the chunk: one descriptor dword -> 32 nibbles -> one
// ds_write_b128), and all four waves read their A operands from it (four ds_read_b128 per tile, conflict-free).  One barrier
// per chunk -- the first LDS form of this kernel had one per tile and lost 14 % to it (profiles/r02h).
// The expansion is software-pipelined over chunks: a thread loads the four descriptor dwords of chunk c + 2 with four
// independent loads through a running pointer at the top of chunk c (whole tiles only: no row guard), and expands them with
// fp4_word (7 vector instructions per dword, no table) at the top of chunk c + 1, so the one wait for them (one vmcnt per
// chunk) comes after a chunk's 64 MFMAs and its barrier.  Until profiles/r23a every tile of the next chunk was a round trip
// of its own -- load, wait, four table reads from LDS, wait, write -- in front of the chunk's first MFMA; the in-order wave
// stood through four global and four LDS latencies per chunk, and the kernel ran well above the matrix time its pattern
// needs (profiles/microbench/mfma_fp4_rate_mi355x.txt).  What is left over after the whole chunks -- up to three whole tiles
// and the frame's partial last tile -- is one tail chunk with guarded loads, loaded and expanded ahead in the same way.
// Every work-group of a pair expands the whole query range it sweeps (7 vector instructions per tile and wave): the four
// groups of a 2000-row frame repeat each other's expansion and save 0.29 GB of traffic per step and one launch.
// ------------------------------------------------------------------------------------------
// The MFMA runs in its block-scaled form with a max-only epilogue: the running best is carried relative to the tile and
// enters the v_max3 chain (8 v_max3 + 1 add = 9 vector instructions per 32 x 32 tile; 37 per query tile and wave with the
// LDS address, beside 16 MFMAs and 4 ds_read_b128).  (The unscaled sub-form measured in profiles/r03h left the tree in
// round 4.)  MFMAs and vector instructions of DIFFERENT waves of a SIMD do overlap: the kernel's own pattern -- chains of four
// FP4 MFMAs and the 16-register max epilogue -- runs at 41.5 cycles per MFMA at three waves per SIMD against 38.8 for bare
// MFMAs (profiles/microbench/mfma_fp4_rate_mi355x.txt).  Inside ONE wave they do not (the software-pipelined epilogue of
// profiles/r03h: 0.232 ms either way), and a wave that waits for memory or LDS issues nothing: what this kernel lost above
// that pace was waiting, not vector work.  The measured pace before and after is in profiles/r23a/README.md.
constexpr int kFuseChunk = 4; // query tiles per chunk: 2 x 4 x 4 KiB = 32 KiB of LDS per work-group

// (Round 4 tried eight wavefronts per work-group -- twice the train rows per work-group, half as many work-groups expanding
// every query tile, 145 instead of 165 VGPRs: 0.213 against 0.190 ms per 499 pairs, profiles/r04b/ab_short_forms_and_options.txt
// row "w8"; the patch is profiles/variants/matcher_8_waves.patch.txt.)
template <int TT>
__global__ __launch_bounds__(kBlock, PS_MFMA_WAVES) void ps_hamming_mfma_fused(const uint32_t *__restrict__ desc,
                                                                const int32_t *__restrict__ nkpts,
                                                                const int32_t *__restrict__ pairs, int cap, int fstride, int tpf,
                                                                int groups, int qsplit, uint32_t *__restrict__ keys)
{
    __shared__ uint4 s_a[2][kFuseChunk][kTileU4];
    const unsigned perPair = (unsigned)(groups * qsplit);
    const unsigned L = xcd_remap(blockIdx.x, gridDim.x);
    const int p = (int)(L / perPair);
    const int inner = (int)(L - (unsigned)p * perPair);
    const int g = inner / qsplit, qs = inner - g * qsplit;
    const int fq = pairs[2 * p], ft = pairs[2 * p + 1]; // query = previous frame, train = current
    const int nq = nkpts[fq], nt = nkpts[ft];
    if (g * (kWavesPerWG * TT * kTileRows) >= nt) return; // whole work-group beyond the train rows
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int tile0 = (g * kWavesPerWG + wave) * TT;
    const int nqTiles = (nq + kTileRows - 1) / kTileRows;
    const int T0 = (int)(((long long)nqTiles * qs) / qsplit), T1 = (int)(((long long)nqTiles * (qs + 1)) / qsplit);

    // B operands: this wave's train tiles, expanded in registers (rows beyond nt repeat the last row; never stored)
    const uint32_t *__restrict__ t32 = desc + (size_t)ft * fstride;
    v4i_t B[TT][4];
#pragma unroll
    for (int i = 0; i < TT; ++i) {
        int t = (tile0 + i) * kTileRows + r;
        t = t < nt ? t : nt - 1;
#pragma unroll
        for (int s = 0; s < 4; ++s) B[i][s] = fp4_from_dword(t32[(size_t)t * 8 + 2 * s + h]);
    }
    v16f_t C;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) C[reg] = kMfmaBase + (float)((1 << 21) + 31 - tile_row(reg, h));
    // Running best of every train column, carried RELATIVE to the tile it meets next: rel = best - cT(T), cT(T) = 16352 - 32 T
    // (see tile_body).  It starts below every valid entry (their patterns are >= 0x4B000000) and grows by 32 per tile, so
    // with at most 512 tiles "no query row seen" stays recognisable as a small value.
    int rel[TT];
#pragma unroll
    for (int i = 0; i < TT; ++i) rel[i] = 0;

    // expansion role of this thread: piece o = s * 64 + h * 32 + r of a tile = dword 2 s + h of row r
    const uint32_t *__restrict__ q32 = desc + (size_t)fq * fstride;
    const int es = tid >> 6, eh = (tid >> 5) & 1, er = tid & 31;
    // The last query tile of a frame may be partial (rows beyond nq must never win: their accumulators start from -1e30).
    // It is taken out of the main loop: left inside, the compiler turns the rare masking into 16 compares + 16 selects for
    // EVERY tile (50 of the 126 vector instructions per tile this kernel had, profiles/r03h).
    const int lastT = (nq & (kTileRows - 1)) ? nqTiles - 1 : -1;
    const bool hasPartial = lastT >= T0 && lastT < T1;
    const int Tm = hasPartial ? lastT : T1; // whole tiles [T0, Tm)
    // The sweep is cut into nFull chunks of kFuseChunk WHOLE tiles (the main loop: unguarded loads through a running pointer)
    // and one tail chunk of the 0..3 whole tiles left over plus the partial tile (guarded loads, outside the loop).
    const int nFull = (Tm - T0) / kFuseChunk;
    const int rem = (Tm - T0) - nFull * kFuseChunk;
    const int nTail = rem + (hasPartial ? 1 : 0);
    const int nChunks = nFull + (nTail > 0 ? 1 : 0);
    const uint32_t *__restrict__ qp = q32 + ((size_t)T0 * kTileRows + er) * 8 + 2 * es + eh; // this thread's dword of the next chunk to load
    // the four descriptor dwords of chunk k, as four independent loads (k ascends by one from call to call)
    auto load_chunk = [&](int k, uint32_t (&W)[kFuseChunk]) {
        if (k < nFull) { // (work-group uniform)
#pragma unroll
            for (int j = 0; j < kFuseChunk; ++j) W[j] = qp[j * (kTileRows * 8)];
            qp += kFuseChunk * kTileRows * 8;
        } else { // the tail: rows beyond the frame are not read (their accumulators start from -1e30 whatever the operand)
#pragma unroll
            for (int j = 0; j < kFuseChunk; ++j) {
                W[j] = 0;
                if (j < nTail && (T0 + nFull * kFuseChunk + j) * kTileRows + er < nq) W[j] = qp[j * (kTileRows * 8)];
            }
        }
    };
    uint32_t kSign = 0x88888888u, kFill = 0x66666666u; // (in registers: see fp4_word)
    asm volatile("" : "+s"(kSign), "+v"(kFill));
    auto expand_chunk = [&](int buf, const uint32_t (&W)[kFuseChunk]) {
#pragma unroll
        for (int j = 0; j < kFuseChunk; ++j)
            s_a[buf][j][tid] = make_uint4(fp4_word(W[j], 0, kSign, kFill), fp4_word(W[j], 1, kSign, kFill),
                                          fp4_word(W[j], 2, kSign, kFill), fp4_word(W[j], 3, kSign, kFill));
    };
    // one query tile against this wave's TT train tiles
    auto tile_body = [&](const uint4 *__restrict__ tile, const v16f_t &Cin) {
        v4i_t A[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const uint4 a = tile[s * 64 + lane];
            A[s].x = (int)a.x; A[s].y = (int)a.y; A[s].z = (int)a.z; A[s].w = (int)a.w;
        }
        // block-scaled MFMA: every product carries 2^9, the accumulator's mantissa is 2^14 (256 - hamming) + (31 - row);
        // adding the tile's cT = 16352 - 32 T would turn it into 2^14 (256 - hamming) + (16383 - query row), whose maximum over
        // rows AND tiles is the nearest query, lowest index first.  The add is not made: the running best is carried less
        // cT instead, enters the v_max3 chain as its 17th value, and moves on to the next tile (cT falls by 32) with one add:
        // 8 v_max3 + 1 add per 32 x 32 tile.
#pragma unroll
        for (int i = 0; i < TT; ++i) {
            v16f_t acc = mfma_fp4s(A[0], B[i][0], Cin);
            acc = mfma_fp4s(A[1], B[i][1], acc);
            acc = mfma_fp4s(A[2], B[i][2], acc);
            acc = mfma_fp4s(A[3], B[i][3], acc);
            int m = imax3(rel[i], fbits(acc[0]), fbits(acc[1]));
#pragma unroll
            for (int e = 2; e < 16; e += 2) m = imax3(m, fbits(acc[e]), fbits(acc[e + 1]));
            rel[i] = m + kTileRows;
        }
    };
    // Software pipeline over chunks: W holds the dwords of the chunk that is expanded NEXT.  At the top of the round of chunk
    // k, chunk k + 1 (loaded a round ago) is expanded into the other LDS buffer; then -- W is free -- chunk k + 2 is loaded
    // with the round's 64 MFMAs and its barrier still ahead: the only wait for it is the first use of W in the next round.
    uint32_t W[kFuseChunk] = {0, 0, 0, 0};
    if (nChunks > 0) {
        load_chunk(0, W);
        expand_chunk(0, W);
    }
    if (nChunks > 1) load_chunk(1, W);
    __syncthreads();
    for (int k = 0; k < nFull; ++k) {
        // (chunk k + 1; in the last round without a tail this writes a buffer nobody reads again)
        expand_chunk((k + 1) & 1, W);
        if (k + 2 < nChunks) load_chunk(k + 2, W);
#pragma unroll 1
        for (int j = 0; j < kFuseChunk; ++j) tile_body(s_a[k & 1][j], C);
        __syncthreads(); // chunk k + 1 is complete, chunk k may be overwritten
    }
    if (nTail > 0) { // (work-group uniform) the tail chunk lies expanded in buffer nFull & 1
#pragma unroll 1
        for (int j = 0; j < rem; ++j) tile_body(s_a[nFull & 1][j], C);
        if (hasPartial) {
            v16f_t Cin = C;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg)
                if (lastT * kTileRows + tile_row(reg, h) >= nq) Cin[reg] = kMfmaNoRow;
            tile_body(s_a[nFull & 1][rem], Cin);
        }
    }
    // the tiles [T0, T1) were met in ascending order: rel is relative to tile T1
    const int cEnd = 16352 - kTileRows * T1;
#pragma unroll
    for (int i = 0; i < TT; ++i) {
        const int t = (tile0 + i) * kTileRows + r;
        uint32_t key = kNoKey;
        if (rel[i] >= 0x4B000000) { // a query row was seen (otherwise rel is at most 32 * 513)
            const int d = (rel[i] + cEnd) & 0x7FFFFF; // 2^14 (256 - hamming) + (16383 - query row)
            key = ((uint32_t)(256 - (d >> 14)) << 16) | (uint32_t)(16383 - (d & 0x3FFF));
        }
        const uint32_t other = (uint32_t)__shfl_xor((int)key, 32, 64); // the other half's 16 rows of every tile
        key = other < key ? other : key;
        if (h == 0 && t < nt) {
            if (qsplit == 1)
                keys[(size_t)p * cap + t] = key;
            else
                atomicMin(&keys[(size_t)p * cap + t], key);
        }
    }
}

} // namespace psdev
