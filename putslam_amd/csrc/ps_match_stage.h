// ps_match_stage.h -- kernels 1 and 2 of the pair pipeline and the stage that runs them: BFMatcher with crossCheck = true
// (reference src/Matcher/matcherOpenCV.cpp:203) over P pairs of a device-resident frame set, then the depth filter and the
// scoring records of RANSAC::estimateTransformation.
//
// Kernel 1  ps_hamming_nn      train -> nearest query (the N x N popcount sweep); its matrix-core twins are ps_matcher_mfma.h's
// Kernel 2  ps_crosscheck_prep OpenCV cross-check, ordered compaction, depth filter, records (ps_pair_records.h)
//
// Host side: run_match_stage picks the matcher by batch size and queues kernels 1 + 2 (the plan is ps_ransac_stage.h's);
// ps_match_hamming256 is the host-pointer form of the match alone.  The keys block and kNoKey are described in ps_matcher_mfma.h.
#pragma once
#include "ps_block.h" // kBlock, xcd_remap, phase_stamp, the flag scans
#include "ps_glue.h"
#include "ps_matcher_mfma.h" // kNoKey; ps_expand_query_fp4 / ps_hamming_mfma(_fused)
#include "ps_pair_records.h" // PrepArgs, RecPtrs, PairRecords
#include "ps_ransac_stage.h" // Plan, rec_ptrs, ensure_records

namespace psdev {

// v_bcnt_u32_b32: popcount(x) + acc in one VALU op (the compiler emits bcnt + add otherwise).
PS_D uint32_t bcnt_acc(uint32_t x, uint32_t acc)
{
    uint32_t r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
    return r;
}

PS_D uint32_t ham_key(const uint4 &a, const uint4 &b, const uint4 &x, const uint4 &y, uint32_t q)
{
    uint32_t d = bcnt_acc(a.x ^ x.x, 0u);
    d = bcnt_acc(a.y ^ x.y, d);
    d = bcnt_acc(a.z ^ x.z, d);
    d = bcnt_acc(a.w ^ x.w, d);
    d = bcnt_acc(b.x ^ y.x, d);
    d = bcnt_acc(b.y ^ y.y, d);
    d = bcnt_acc(b.z ^ y.z, d);
    d = bcnt_acc(b.w ^ y.w, d);
    return (d << 16) | q; // lexicographic (distance, query): min == strict '<' scan in ascending q
}

// ------------------------------------------------------------------------------------------
// Kernel 1.  cv::batchDistance(train, query, K=1) inside BFMatcher's cross-check
// (reference call site src/Matcher/matcherOpenCV.cpp:203): for each train row the nearest
// query row, ties to the lowest query index.
// One lane owns TPL train descriptors in VGPRs (8 dwords each).  The query rows are
// wave-uniform, so they are fetched with scalar loads (s_load_dwordx8) into SGPRs and feed
// v_xor/v_bcnt directly: no LDS traffic, no bank conflicts, 18 VALU ops per pair.
// grid = tiles * qsplit * P work-groups in XCD-aware order.  qsplit > 1 splits the query range across workgroups (few pairs,
// many CUs) and merges with atomicMin on the packed key.
// ------------------------------------------------------------------------------------------
template <int TPL>
__global__ __launch_bounds__(kBlock) void ps_hamming_nn(const uint4 *__restrict__ desc,
                                                        const int32_t *__restrict__ nkpts,
                                                        const int32_t *__restrict__ pairs, int cap, int fstride, int tiles,
                                                        int qsplit, uint32_t *__restrict__ keys)
{
    const unsigned perPair = (unsigned)(tiles * qsplit);
    const unsigned L = xcd_remap(blockIdx.x, gridDim.x);
    const int p = (int)(L / perPair);
    const int inner = (int)(L - (unsigned)p * perPair);
    const int fq = pairs[2 * p], ft = pairs[2 * p + 1]; // query = previous frame, train = current
    const int nq = nkpts[fq], nt = nkpts[ft];
    const int tile = inner / qsplit, qs = inner - tile * qsplit;
    const int t0 = tile * (kBlock * TPL);
    if (t0 >= nt) return;
    const int q0 = (int)(((long long)nq * qs) / qsplit), q1 = (int)(((long long)nq * (qs + 1)) / qsplit);

    // (fstride: uint4 units between consecutive frames' descriptor blocks -- cap * 2 for the dense frame set, the packed
    // frame's stride when descriptors and points of a frame lie together, PsFrameSet::descFrameStride)
    const uint4 *__restrict__ tdesc = desc + (size_t)ft * fstride;
    const uint4 *__restrict__ qdesc = desc + (size_t)fq * fstride;

    uint4 a[TPL], b[TPL];
    uint32_t best[TPL];
#pragma unroll
    for (int i = 0; i < TPL; ++i) {
        int t = t0 + i * kBlock + threadIdx.x;
        int tc = t < nt ? t : nt - 1;
        a[i] = tdesc[2 * tc];
        b[i] = tdesc[2 * tc + 1];
        best[i] = kNoKey;
    }
    int q = q0;
    for (; q + 4 <= q1; q += 4) {
        uint4 x0 = qdesc[2 * q], y0 = qdesc[2 * q + 1];
        uint4 x1 = qdesc[2 * q + 2], y1 = qdesc[2 * q + 3];
        uint4 x2 = qdesc[2 * q + 4], y2 = qdesc[2 * q + 5];
        uint4 x3 = qdesc[2 * q + 6], y3 = qdesc[2 * q + 7];
#pragma unroll
        for (int i = 0; i < TPL; ++i) {
            best[i] = min(best[i], ham_key(a[i], b[i], x0, y0, (uint32_t)q));
            best[i] = min(best[i], ham_key(a[i], b[i], x1, y1, (uint32_t)q + 1));
            best[i] = min(best[i], ham_key(a[i], b[i], x2, y2, (uint32_t)q + 2));
            best[i] = min(best[i], ham_key(a[i], b[i], x3, y3, (uint32_t)q + 3));
        }
    }
    for (; q < q1; ++q) {
        uint4 x0 = qdesc[2 * q], y0 = qdesc[2 * q + 1];
#pragma unroll
        for (int i = 0; i < TPL; ++i) best[i] = min(best[i], ham_key(a[i], b[i], x0, y0, (uint32_t)q));
    }
#pragma unroll
    for (int i = 0; i < TPL; ++i) {
        int t = t0 + i * kBlock + threadIdx.x;
        if (t < nt) {
            if (qsplit == 1)
                keys[(size_t)p * cap + t] = best[i];
            else
                atomicMin(&keys[(size_t)p * cap + t], best[i]);
        }
    }
}

// ------------------------------------------------------------------------------------------
// Kernel 2.  Cross-check + ordered compaction (BFMatcher with crossCheck=true) followed by the
// depth filter of RANSAC::estimateTransformation (RANSAC.cpp:65-74) and record building.
// One workgroup per pair; best[q] lives in LDS (cap x 4 B).
// ------------------------------------------------------------------------------------------
// BLOCK = 1024 is the low-latency form for a handful of pairs (one work-group per pair either way).
template <bool WITH_RECORDS, int BLOCK = kBlock>
__global__ __launch_bounds__(BLOCK) void ps_crosscheck_prep(const float *__restrict__ pts,
                                                             const int32_t *__restrict__ nkpts,
                                                             const int32_t *__restrict__ pairs,
                                                             uint32_t *__restrict__ keys, PrepArgs a,
                                                             PsDMatch *__restrict__ matches,
                                                             int32_t *__restrict__ numMatches, RecPtrs rec,
                                                             int32_t *__restrict__ mvalid, float2 *__restrict__ cmaxOut,
                                                             unsigned long long *__restrict__ stamps)
{
    extern __shared__ __align__(16) uint32_t s_best[];
    phase_stamp(stamps, 0);
    __shared__ int s_wsum[2 * (BLOCK / 64)];
    __shared__ float2 s_red[BLOCK / 64];
    const int p = blockIdx.x;
    const int cap = a.cap;
    const int fq = pairs[2 * p], ft = pairs[2 * p + 1];
    const int nq = nkpts[fq], nt = nkpts[ft];
    // (the thread's first two keys are on their way while best[] is initialised: they come from the matcher's launch)
    uint32_t k0 = kNoKey, k1 = kNoKey;
    if ((int)threadIdx.x < nt) k0 = keys[(size_t)p * cap + threadIdx.x];
    if ((int)threadIdx.x + BLOCK < nt) k1 = keys[(size_t)p * cap + threadIdx.x + BLOCK];
    for (int q = threadIdx.x; q < nq; q += BLOCK) s_best[q] = kNoKey;
    __syncthreads();
    // step 2 of the cross-check: query q keeps the closest train row among those that chose it,
    // ties to the lowest train index (strict '<' while scanning t ascending).
    for (int t = threadIdx.x; t < nt; t += BLOCK) {
        uint32_t key = t < BLOCK ? k0 : (t < 2 * BLOCK ? k1 : keys[(size_t)p * cap + t]);
        if (key != kNoKey) {
            uint32_t q = key & 0xFFFFu, d = key >> 16;
            atomicMin(&s_best[q], (d << 16) | (uint32_t)t);
            keys[(size_t)p * cap + t] = kNoKey; // the block is all-ones at rest: the next call's matcher merges with atomicMin
        }
    }
    __syncthreads();
    phase_stamp(stamps, 1); // best[q] built
    const float *pp = pts + (size_t)fq * a.ptsStride; // (floats between consecutive frames' point blocks: cap * 3 when dense)
    const float *cp = pts + (size_t)ft * a.ptsStride;
    int base = 0;
    // one candidate per thread and trip; the next trip's key and points are fetched before this trip's scan, so that the
    // gather's latency (the points were written by another launch: nothing is cached) runs beside it instead of in front of
    // every trip (a single pair with 1024 threads makes two trips)
    struct Cand {
        uint32_t key;
        float px, py, pz, cx, cy, cz;
    };
    auto fetch = [&](int q, Cand &c) {
        c.key = (q < nq) ? s_best[q] : kNoKey;
        c.px = c.py = c.pz = c.cx = c.cy = c.cz = 0.0f;
        if (WITH_RECORDS && c.key != kNoKey) {
            const int t = (int)(c.key & 0xFFFFu);
            c.px = pp[3 * q]; c.py = pp[3 * q + 1]; c.pz = pp[3 * q + 2];
            c.cx = cp[3 * t]; c.cy = cp[3 * t + 1]; c.cz = cp[3 * t + 2];
        }
    };
    PairRecords pr(a, rec, p, WITH_RECORDS);
    Cand cur;
    fetch((int)threadIdx.x, cur);
    int trip = 0;
    for (int q0 = 0; q0 < nq; q0 += BLOCK, ++trip) {
        const int q = q0 + threadIdx.x;
        Cand nxt;
        nxt.key = kNoKey;
        nxt.px = nxt.py = nxt.pz = nxt.cx = nxt.cy = nxt.cz = 0.0f;
        if (q0 + BLOCK < nq) fetch(q + BLOCK, nxt);
        const uint32_t key = cur.key;
        const bool has = key != kNoKey;
        const int t = (int)(key & 0xFFFFu);
        const float px = cur.px, py = cur.py, pz = cur.pz, cx_ = cur.cx, cy_ = cur.cy, cz_ = cur.cz;
        const bool ok = WITH_RECORDS && has && match_depth_ok(px, py, pz, cx_, cy_, cz_);
        // both ordered compactions (cross-check survivors; depth-valid ones among them) with one barrier
        int pos, total, vpos, vtotal;
        block_scan_flags2<BLOCK, false>(has, ok, pos, total, vpos, vtotal, s_wsum, trip);
        if (has) {
            PsDMatch m;
            m.queryIdx = q;
            m.trainIdx = t;
            m.imgIdx = 0;
            m.distance = (float)(key >> 16);
            matches[(size_t)p * cap + base + pos] = m;
        }
        if (WITH_RECORDS) pr.add(ok, vpos, vtotal, base + pos, q, t, px, py, pz, cx_, cy_, cz_);
        base += total;
        cur = nxt;
    }
    phase_stamp(stamps, 2); // matches compacted, records written
    if (WITH_RECORDS) pr.finish<BLOCK>(s_red, mvalid, cmaxOut);
    if (threadIdx.x == 0) numMatches[p] = base;
    phase_stamp(stamps, 3); // bounds, split operands, counters cleared
}

} // namespace psdev

namespace {

constexpr int kMfmaTT = 4;       // train tiles per wave of the MFMA matcher (ps_hamming_mfma<TT>, ps_matcher_mfma.h)

// The matcher forms that merge with atomicMin start from an all-ones keys block (see PsContext::keysCleanPtr).
int keys_clean(PsContext *ctx, size_t bytes)
{
    if (ctx->keysCleanPtr == ctx->keys.p && ctx->keysCleanBytes >= bytes) return PS_OK;
    PS_HIP(hipMemsetAsync(ctx->keys.p, 0xFF, ctx->keys.cap, ctx->stream));
    ctx->keysCleanPtr = ctx->keys.p;
    ctx->keysCleanBytes = ctx->keys.cap;
    return PS_OK;
}

// Kernel 2 with (REC) or without the scoring records, BLK threads per work-group.
template <bool REC, int BLK>
void launch_prep(PsContext *ctx, const PsFrameSet &fs, const int32_t *dPairs, int P, const PrepArgs &pa, const RecPtrs &rp,
                 PsDMatch *dMatches, int32_t *dNumMatches)
{
    hipLaunchKernelGGL((ps_crosscheck_prep<REC, BLK>), dim3((unsigned)P), dim3(BLK), (size_t)fs.maxKpts * sizeof(uint32_t), ctx->stream,
                       fs.pts, fs.nkpts, dPairs, (uint32_t *)ctx->keys.p, pa, dMatches, dNumMatches, rp, (int32_t *)ctx->mvalid.p,
                       (float2 *)ctx->cmax.p, ctx->stampsOn ? (unsigned long long *)ctx->stamps.p : (unsigned long long *)nullptr);
}

// Kernels 1 + 2 for P pairs of a device-resident frame set: kernel 2 writes the records of plan `pl`, or matches only
// (pl = null).
int run_match_stage(PsContext *ctx, const PsFrameSet &fs, const int32_t *dPairs, int P, const Plan *pl, PsDMatch *dMatches,
                    int32_t *dNumMatches, int slot0)
{
    const int cap = fs.maxKpts;
    FrameStrides strides; // (PsFrameSet, ABI 2: dense unless the frames keep descriptors and points together; no points: ps_match_hamming256)
    if (int rc = frame_strides(ctx, fs, true, fs.pts != nullptr, "frame set", strides)) return rc;
    const int fstrideDw = strides.descDwords();
    PrepArgs pa = pl ? pl->pa : PrepArgs{};
    if (!pl) pa.cap = cap;
    pa.ptsStride = strides.ptsFloats();
    PS_ENSURE(ctx->keys, (size_t)P * cap * sizeof(uint32_t));
    PS_ENSURE(ctx->mvalid, (size_t)P * sizeof(int32_t));
    PS_ENSURE(ctx->cmax, (size_t)P * sizeof(float2));
    if (pl) {
        int rc = ensure_records(ctx, (size_t)P, (size_t)cap);
        if (rc != PS_OK) return rc;
    }
    // by batch size: VALU sweep 1.85 us, MFMA sweep 0.43 us per 2000 x 2000 pair on a full chip, + ~7 us for the extra launch
    const bool useMfma = ctx->matcher == 1 || (ctx->matcher == 2 && (double)P * cap * cap > 2.0e7);
    ctx->matcherUsed = useMfma ? 1 : 0;
    const size_t keyBytes = (size_t)P * cap * sizeof(uint32_t);
    // from the matcher's launch until kernel 2 has been queued behind it the keys block is in use; kernel 2 leaves what it
    // read all-ones again, so a block that was clean before this call is clean after it
    const size_t cleanBefore = ctx->keysCleanPtr == ctx->keys.p ? ctx->keysCleanBytes : 0;
    struct KeysInUse {
        PsContext *c;
        size_t restore;
        bool done = false;
        ~KeysInUse() { c->keysCleanBytes = done ? restore : 0; }
    } keysInUse{ctx, cleanBefore};
    if (useMfma) {
        // matrix-core form: expand every pair's query frame to FP4 once, then the MFMA sweep
        constexpr int TT = kMfmaTT;
        const int tpf = (cap + kTileRows - 1) / kTileRows;
        const int groups = (tpf + kWavesPerWG * TT - 1) / (kWavesPerWG * TT);
        int qsplit = pick_split((long long)P * groups, tpf, 1, tpf);
        if (ctx->forceQsplit > 0) qsplit = ctx->forceQsplit < tpf ? ctx->forceQsplit : tpf;
        if (ctx->matcherFused) {
            // fused expansion: every work-group of a query split expands its own share of the query tiles, so a split only
            // pays when the groups do not fill the chip by themselves; the splits merge with atomicMin on an all-ones keys block
            // (kept so by kernel 2: keys_clean)
            if (ctx->forceQsplit <= 0 && (long long)P * groups >= 1024) qsplit = 1;
            if (qsplit > 1) {
                int rc = keys_clean(ctx, keyBytes);
                if (rc != PS_OK) return rc;
                keysInUse.restore = ctx->keysCleanBytes;
            }
            tick(ctx, 5, false);
            hipLaunchKernelGGL(ps_hamming_mfma_fused<TT>, dim3((unsigned)(groups * qsplit) * (unsigned)P), dim3(kBlock), 0,
                               ctx->stream, (const uint32_t *)fs.desc, fs.nkpts, dPairs, cap, fstrideDw, tpf, groups, qsplit,
                               (uint32_t *)ctx->keys.p);
            tick(ctx, 5, true);
            PS_HIP(hipGetLastError());
        } else {
        PS_ENSURE(ctx->xq, (size_t)P * tpf * kTileU4 * sizeof(uint4));
        int xchunks = tpf < 8 ? tpf : 8;
        if ((long long)P * xchunks < 1024) xchunks = tpf < 64 ? tpf : 64;
        tick(ctx, 4, false);
        hipLaunchKernelGGL(ps_expand_query_fp4, dim3((unsigned)xchunks * (unsigned)P), dim3(kBlock), 0, ctx->stream,
                           (const uint32_t *)fs.desc, fs.nkpts, dPairs, cap, fstrideDw, tpf, xchunks, (uint4 *)ctx->xq.p,
                           qsplit > 1 ? (uint32_t *)ctx->keys.p : (uint32_t *)nullptr); // also clears the keys
        tick(ctx, 4, true);
        tick(ctx, 5, false);
        hipLaunchKernelGGL(ps_hamming_mfma<TT>, dim3((unsigned)(groups * qsplit) * (unsigned)P), dim3(kBlock), 0,
                           ctx->stream, (const uint32_t *)fs.desc, fs.nkpts, dPairs, cap, fstrideDw, tpf, groups, qsplit,
                           (const uint4 *)ctx->xq.p, (uint32_t *)ctx->keys.p);
        tick(ctx, 5, true);
        PS_HIP(hipGetLastError());
        }
    } else {
        constexpr int TPL = 2;
        const int tiles = (cap + kBlock * TPL - 1) / (kBlock * TPL);
        // single pair: 500 work-groups of 16 query rows (84.1 us per pair against 84.6 with 64 splits of 31 rows and 85.6
        // with 250 of 8, profiles/r04g/ab_latency.txt)
        int qsplit = pick_split((long long)P * tiles, 128, 16, cap);
        if (ctx->forceQsplit > 0) qsplit = ctx->forceQsplit;
        if (qsplit > 1) {
            int rc = keys_clean(ctx, keyBytes);
            if (rc != PS_OK) return rc;
            keysInUse.restore = ctx->keysCleanBytes;
        }
        tick(ctx, slot0, false);
        hipLaunchKernelGGL(ps_hamming_nn<TPL>, dim3((unsigned)(tiles * qsplit) * (unsigned)P), dim3(kBlock), 0, ctx->stream,
                           (const uint4 *)fs.desc, fs.nkpts, dPairs, cap, strides.descUint4(), tiles, qsplit, (uint32_t *)ctx->keys.p);
        tick(ctx, slot0, true);
        PS_HIP(hipGetLastError());
    }
    tick(ctx, slot0 + 1, false);
    const bool wide = P <= kWidePairs; // a handful of pairs: 1024-thread work-groups shorten the per-pair serial walk
    const auto prep = pl ? (wide ? launch_prep<true, 1024> : launch_prep<true, kBlock>)
                         : (wide ? launch_prep<false, 1024> : launch_prep<false, kBlock>);
    prep(ctx, fs, dPairs, P, pa, pl ? rec_ptrs(ctx, pl->score) : RecPtrs{}, dMatches, dNumMatches);
    tick(ctx, slot0 + 1, true);
    PS_HIP(hipGetLastError());
    keysInUse.done = true;
    return PS_OK;
}

} // namespace

extern "C" {

// ---------------------------------------------------------------------------------------------
int ps_match_hamming256(PsContext *ctx, const uint8_t *query, int nq, size_t qstep, const uint8_t *train, int nt,
                        size_t tstep, PsDMatch *out, int *nout)
{
    int rc = bind(ctx);
    if (rc) return rc;
    TimingOff toff(ctx);
    if (nout) *nout = 0;
    if (!out || !nout || nq < 0 || nt < 0 || (nq > 0 && !query) || (nt > 0 && !train))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_match_hamming256: bad argument");
    if ((nq > 0 && qstep < PS_DESC_BYTES) || (nt > 0 && tstep < PS_DESC_BYTES))
        return fail(ctx, PS_ERR_UNSUPPORTED, "descriptor rows must be 32 bytes (ORB/LDB); float descriptors are out of scope");
    if (nq > PS_MAX_KPTS || nt > PS_MAX_KPTS) return fail(ctx, PS_ERR_UNSUPPORTED, "more than PS_MAX_KPTS rows");
    if (nq == 0 || nt == 0) return PS_OK; // BFMatcher on an empty side: no matches
    int cap = nq > nt ? nq : nt;
    PS_ENSURE(ctx->sDesc, (size_t)2 * cap * 32);
    PS_ENSURE(ctx->sNk, 2 * sizeof(int32_t) + 2 * sizeof(int32_t));
    PS_ENSURE(ctx->sMatches, (size_t)cap * sizeof(PsDMatch));
    PS_ENSURE(ctx->sNumM, sizeof(int32_t));
    uint8_t *dDesc = (uint8_t *)ctx->sDesc.p;
    PS_HIP(hipMemcpy2DAsync(dDesc, 32, query, qstep, 32, (size_t)nq, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpy2DAsync(dDesc + (size_t)cap * 32, 32, train, tstep, 32, (size_t)nt, hipMemcpyHostToDevice,
                            ctx->stream));
    int32_t hostMeta[4] = {nq, nt, 0, 1}; // nkpts[2], pair (0,1)
    PS_HIP(hipMemcpyAsync(ctx->sNk.p, hostMeta, sizeof hostMeta, hipMemcpyHostToDevice, ctx->stream));
    PsFrameSet fs;
    fs.desc = dDesc;
    fs.pts = nullptr;
    fs.nkpts = (const int32_t *)ctx->sNk.p;
    fs.numFrames = 2;
    fs.maxKpts = cap;
    fs.descFrameStride = fs.ptsFrameStride = 0;
    rc = run_match_stage(ctx, fs, (const int32_t *)ctx->sNk.p + 2, 1, nullptr, (PsDMatch *)ctx->sMatches.p, (int32_t *)ctx->sNumM.p, 0);
    if (rc) return rc;
    int32_t n = 0;
    PS_HIP(hipMemcpyAsync(&n, ctx->sNumM.p, sizeof n, hipMemcpyDeviceToHost, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream));
    if (n > 0) {
        PS_HIP(hipMemcpyAsync(out, ctx->sMatches.p, (size_t)n * sizeof(PsDMatch), hipMemcpyDeviceToHost, ctx->stream));
        PS_HIP(hipStreamSynchronize(ctx->stream));
    }
    *nout = n;
    return PS_OK;
}

} // extern "C"
