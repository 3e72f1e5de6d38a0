// ps_stream_async.h -- the PIPELINED streaming form of Matcher::match (include/putslam_hip.h: ps_vo_stream_configure_async,
// _push_async, _push_many, _flush, _pop_many, _pop).  Included by ps_capi.hip behind ps_stream_push.h (it uses that header's
// PsVoStream and ps_capi.hip's plan and stages).  Layout of this file: the state (shared, ring form, mini form), a chunk's launch
// (begin, the form's launches, commit), the one push path, configure, the C entry points.
//
// Call shape served: reference src/Matcher/matcher.cpp:452-516 (one frame per call, the previous frame kept as state) in the
// loop of src/PUTSLAM/PUTSLAM.cpp:677-740.  The synchronous ps_vo_stream_push pays a copy in, four kernels, a copy out and a
// synchronisation per frame (0.08 ms: 12.5 k frames/s); here frames are collected into chunks, each chunk is one batched call
// (ps_vo_pairs_device's launches) on one of several lanes, and the results are returned with a lag:
//
//   host frames --(copy stream: SDMA uploads)--> ring of frames in HBM --(lane k % lanes: kernels 1-4)--(download stream)--> pinned block --> pop
//
//   * the copy stream carries ONLY the two large uploads of every chunk (descriptors, points), which the runtime gives to an
//     SDMA engine: back to back they keep the link at 48 GB/s of its 55.  The chunk's small meta block (pair list, row counts)
//     is fetched by a one-work-group kernel on the lane's own stream from mapped pinned memory: as a third hipMemcpyAsync on the
//     copy stream it was a blit kernel between SDMA transfers, and every change of engine left the link idle for 60 us
//     (rocprofv3 timeline, profiles/r05a/stream_trace).  Uploads as kernels over mapped pinned memory reach the link rate too
//     (profiles/microbench/h2d_kernel.hip) but slow the kernels they run beside by 3 - 10 x (profiles/r05b/stream_trace: their
//     outstanding host reads fill the L2's request queues); SDMA transfers do not.
//
//   * places: a chunk needs a place (meta block, device + pinned result blocks, events), not a lane: there are lanes + `ahead`
//     of them (option "stream_ahead"; default: six places in all), and chunk k is LAUNCHED at once on lane k % lanes -- behind that lane's running
//     chunk if it has one.  With one place per lane a lane idled from the end of its chunk's last kernel through the download,
//     the host's pop, the next chunk's upload and the copy-stream -> lane dependency (300 - 500 us of a chunk's ~ 800,
//     profiles/r05h/timeline_ahead0.txt); now its next chunk's launches are already in its stream.
//   * ring: (lanes + ahead + 2) x chunkFrames + lanes + ahead frame slots.  A chunk's frames are contiguous in it (a chunk that
//     would not fit before the end starts at slot 0 again); the frame before the chunk's first one is still resident, so pair
//     (previous chunk's last frame, this chunk's first frame) needs no second upload.  No slot that is still read is overwritten,
//     with no device-side wait: the count is ps_stream_ledger.h's (THE REUSE INVARIANT), which also keeps every integer of the
//     pipeline -- places, the staging areas' rotation, the ring cursor, pair numbers, epochs -- and changes them in one place,
//     when a chunk has been queued completely.
//   * lane = a private PsContext (stream + scratch arena).  Consecutive chunks go to consecutive lanes, so one chunk's matrix-core
//     Hamming sweep runs beside another's vector scoring sweep, as bench.py's sub-batch chains do.  The pinned result block of a
//     place changes hands at the pop: the caller reads it until the next pop, the place continues with the spare one -- so a
//     place is free the moment its results are popped.
//   * per chunk: 2 uploads, the meta kernel, the batched call's launches, 1 download (5 for a partly filled chunk); uploads are
//     in stream order, so the halo frame needs no event of its own.
//   * results are those of ONE ps_vo_pairs_device call over the whole sequence: pair k draws from cfg->seed + k.
#pragma once
#include "ps_stream_ledger.h" // every integer of the pipeline and the rule that makes reuse safe; the result block's layout
#include "ps_stream_push.h"   // PsVoStream, ps_copy_segments

namespace psdev {

// Small chunks of the pipelined stream (chunkFrames <= 4: ps_stream_async.h, "mini" chunks): everything that changes from chunk to
// chunk travels as DATA through this block, so that a place's whole chunk -- frames in, kernels 1 - 4, results out -- is one
// captured hipGraph.  The host fills it in the place's pinned meta block; ps_mini_copy_in copies it to the device meta block,
// which the kernels behind it read (row counts, pair list, seed).
constexpr int kMiniFrames = 4;
struct MiniMeta {
    int32_t pairs[2 * kMiniFrames]; // the chunk's pairs in the place's private frame set: slot 0 = the previous frame (halo), 1 .. n = the chunk's
    int32_t nk[kMiniFrames + 1];    // row counts of the private frames
    int32_t n, first, pad;          // frames in the chunk; 1 = its first frame has no predecessor (slot 0 is not copied)
    unsigned long long seed;        // hypothesis seed of the chunk's first pair (cfg->seed + its number in the stream)
    const uint8_t *src[kMiniFrames + 1]; // device views of the pinned packed frames [cap x 32 B][cap x 12 B]: [0] the halo, [1 .. n] the chunk's
};

// Frames of a mini chunk from pinned host memory into the place's private frame set (packed layout, `stride` bytes per frame),
// and the meta block with them.  grid = (kMiniFrames + 1) x groups work-groups: frame f is swept by `groups` of them.  The reads go
// over the link: 88 KB per 2000-keypoint frame, a few microseconds (the synchronous ps_vo_stream_push moves its frame the same way).
__global__ void __launch_bounds__(256) ps_mini_copy_in(const MiniMeta *__restrict__ hm, MiniMeta *__restrict__ dm, uint8_t *__restrict__ frames,
                                                       int cap, unsigned long long stride, int groups)
{
    if (blockIdx.x == 0 && threadIdx.x < sizeof(MiniMeta) / 4)
        reinterpret_cast<uint32_t *>(dm)[threadIdx.x] = reinterpret_cast<const uint32_t *>(hm)[threadIdx.x];
    const int f = (int)(blockIdx.x / (unsigned)groups), g = (int)(blockIdx.x % (unsigned)groups);
    const int n = hm->n, first = hm->first;
    if (f > n || (f == 0 && first)) return;
    const int rows = hm->nk[f];
    // (the frame's address comes out of memory: told to be a global address, or the compiler emits FLAT loads for it)
    typedef unsigned __attribute__((ext_vector_type(4))) u4v_t;
    typedef const u4v_t __attribute__((address_space(1))) *gu4_t;
    typedef const uint32_t __attribute__((address_space(1))) *gu32_t;
    const uintptr_t src = reinterpret_cast<uintptr_t>(hm->src[f]);
    uint8_t *__restrict__ dst = frames + (size_t)f * stride;
    const size_t t0 = (size_t)g * blockDim.x + threadIdx.x, step = (size_t)groups * blockDim.x;
    { // descriptors: rows x 32 bytes, 16 per lane
        gu4_t sv = (gu4_t)src;
        u4v_t *__restrict__ dv = reinterpret_cast<u4v_t *>(dst);
        for (size_t i = t0; i < (size_t)rows * 2; i += step) dv[i] = sv[i];
    }
    { // points: rows x 12 bytes behind the cap x 32 descriptor bytes, 4 per lane
        gu32_t sv = (gu32_t)(src + (size_t)cap * 32);
        uint32_t *__restrict__ dv = reinterpret_cast<uint32_t *>(dst + (size_t)cap * 32);
        for (size_t i = t0; i < (size_t)rows * 3; i += step) dv[i] = sv[i];
    }
}

// Results of a chunk of the pipelined stream written straight into the lane's mapped pinned block, only what the caller asked
// for (PsStreamResults): mode 1 = the INLIER matches of every pair in input order (what Matcher::match hands back,
// matcher.cpp:452-516: `inlierMatches`) + pose + stats + match count; mode 2 = pose + stats + match count.  One work-group per
// pair; ordered compaction by one ballot-prefix scan per 256 matches.  The writes go over the host link: 12 KB instead of 34 KB
// per 2000-keypoint pair in mode 1, 108 bytes in mode 2.
__global__ __launch_bounds__(kBlock) void ps_pack_results_to_host(const PsDMatch *__restrict__ matches,
                                                                  const int32_t *__restrict__ numMatches,
                                                                  const uint8_t *__restrict__ mask, const float *__restrict__ pose,
                                                                  const PsRansacStats *__restrict__ stats, int cap, int mode,
                                                                  PsDMatch *__restrict__ hMatches, float *__restrict__ hPose,
                                                                  PsRansacStats *__restrict__ hStats, int32_t *__restrict__ hNum)
{
    __shared__ int s_w[2 * (kBlock / 64)];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int n = numMatches[p];
    if (tid < 16) hPose[(size_t)p * 16 + tid] = pose[(size_t)p * 16 + tid];
    if (tid == 0) {
        hStats[p] = stats[p];
        hNum[p] = n;
    }
    if (mode != 1) return;
    const uint4 *__restrict__ src = reinterpret_cast<const uint4 *>(matches + (size_t)p * cap);
    uint4 *__restrict__ dst = reinterpret_cast<uint4 *>(hMatches + (size_t)p * cap);
    const uint8_t *__restrict__ mk = mask + (size_t)p * cap;
    int base = 0, trip = 0;
    for (int i0 = 0; i0 < n; i0 += kBlock, ++trip) {
        const int i = i0 + tid;
        const bool in = i < n && mk[i] != 0;
        int pos, total, posB, totalB;
        block_scan_flags2<kBlock, false>(in, false, pos, total, posB, totalB, s_w, trip);
        if (in) dst[base + pos] = src[i];
        base += total;
    }
}

} // namespace psdev

// One chunk's place in the pipeline: meta block, device and pinned result blocks, events.  There are lanes + ahead of them; a
// chunk takes the next one and runs on the next LANE (a private PsContext: stream + scratch arena) in turn, so each lane's
// stream can hold a chunk that runs and further ones queued behind it.  (Whether a place is taken, and by which pairs: the ledger.)
struct AsyncLane {
    PsContext *ctx = nullptr; // the lane context this place's chunk was launched on (not owned)
    Buf meta;                 // device: int32 [2 * B] pair list, then [ringFrames] row counts (mini: a psdev::MiniMeta)
    int32_t *hmeta = nullptr; // pinned mirror of it
    Buf res;                  // device: the chunk's result block (psledger::ResLayout)
    uint8_t *hres = nullptr;  // pinned mirror of it
    int32_t *hmetaDev = nullptr; // device views of the pinned blocks (hipHostGetDevicePointer)
    uint8_t *hresDev = nullptr;
    hipEvent_t evDone = nullptr; // behind the chunk's download
    // ---- ring form
    hipEvent_t evRun = nullptr;  // behind the chunk's kernels
    // ---- mini form: the place's private frames [1 + B] in the packed layout (slot 0 = the frame before the chunk's first
    // one), its chunk as a captured graph, and the arena generation of its lane the graph's pointers belong to
    Buf frames;
    hipGraphExec_t gexec = nullptr;
    unsigned long long gexecGen = 0;
    Plan plan;                  // the plan of the place's full chunk (parameters are fixed per configure), valid while ...
    unsigned long long planGen = 0; // ... its lane's arena is the one it was made with (0 = none)
};

// The ring form's own: frames travel host -> ring over the copy stream, results come back over the copy-out stream.
struct AsyncRing {
    std::vector<hipEvent_t> upEv; // one upload event per staging area (Ledger::next_area)
    Buf desc, pts;                // the ring (packed frames: `desc` holds ringFrames x packStride bytes, `pts` is unused)
    std::vector<int32_t> nk;      // row counts of the ring's slots (host-authoritative; every chunk uploads a snapshot)
    hipStream_t copyStream = nullptr;    // uploads
    hipStream_t copyOutStream = nullptr; // downloads
    bool downloadsOnLane = false; // downloads queued on the lane's own stream instead of the copy-out stream: when the
                                  // process has few hardware queues (GPU_MAX_HW_QUEUES < lanes + 6), or forced either
                                  // way by PUTSLAM_HIP_STREAM_DOWNLOADS_ON_LANE=0|1
    // The block a pop hands to the caller changes hands instead of keeping its lane busy: the lane takes the spare pinned block
    // and is free at once (round 5's first form held the lane until the NEXT pop: of four lanes three computed).  Pops are in
    // order and a view lives until the next pop, so one block is held at any time.
    uint8_t *spareHres = nullptr, *spareHresDev = nullptr; // free pinned result block (+ its device view)
    uint8_t *heldHres = nullptr, *heldHresDev = nullptr;   // the block the caller's view points into (null: no view)
};

// Small chunks (chunkFrames <= 4, the reference's own call shape at 1: src/Matcher/matcher.cpp:452-516): a chunk is launch-bound
// -- two uploads, a meta kernel, six or seven launches, an event pair and a download, 85 us of host and queue time for 55 us of
// kernels: round 5's pipeline was no faster than the synchronous push there.  In this form every place owns a private frame set
// and its whole chunk is ONE captured hipGraph (frames in by a copy kernel from the pinned staging area, kernels 1 - 4, results
// out by a kernel into the place's pinned block); what changes between chunks -- row counts, the seed, where the frames lie --
// travels as data (psdev::MiniMeta).  No ring, no copy streams, no cross-lane dependency: the halo frame is read again from
// the previous chunk's staging slot.
struct AsyncMini {
    // Replaying a place's chunk from its graph is OFF by default: on this runtime hipGraphLaunch of the seven-node graph costs the
    // host more than the seven launches and the lanes' graphs run less side by side -- 20.9 k frames/s at 322 us of lag against
    // 25.1 k at 209 us with ordinary launches (demos/cpp/demo_latency (d), profiles/r06h/mini_chunks.txt).  PUTSLAM_HIP_STREAM_GRAPH=1
    // turns it on (tests run both).
    bool graphs = false;
    long long graphLaunches = 0;         // chunks replayed from a graph (option "stream_graph_launches", read only)
    std::vector<uint8_t *> stagePoolDev; // device views of the staging areas (the copy-in kernel reads them)
    // the stream's latest frame, which the next chunk reads as its previous one: in its chunk's staging slot, in the caller's
    // pinned memory, or -- a lone first frame, which takes no place and therefore no area -- in a pinned block of its own, written
    // again only behind the chunk that read it
    const uint8_t *haloDev = nullptr;
    int haloNk = 0;
    bool haloIsLone = false;
    uint8_t *loneHost = nullptr, *loneDev = nullptr;
    hipEvent_t loneReadEv = nullptr; // behind the chunk that read that block as its previous frame
    bool loneReadPending = false;
    std::vector<unsigned long long> laneWarmGen; // per lane: arena generation an un-captured full chunk has run with (0 = none)
    std::vector<uint8_t> viewBuf;                // pop_many's copy of a chunk's results (its place is free at once)
};

struct PsVoAsync {
    psledger::Ledger led;
    // ---- both forms
    psledger::ResLayout res;
    PsRansacParams prm{};
    PsRansacConfig cfg{};
    float K[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    bool haveK = false;
    int resultMode = 0;               // PsStreamResults
    bool packed = false;              // PS_FRAMES_PACKED: a frame's descriptors and points lie together, in the ring as on the
    size_t packStride = 0;            // host: ONE upload per chunk (mini chunks: always, one block per frame for the copy-in kernel)
    std::vector<PsContext *> laneCtx; // the lanes (owned)
    std::vector<AsyncLane> lane;      // the lanes + ahead places, taken in ring order
    std::vector<uint8_t *> stagePool; // one pinned staging area per Ledger::next_area for frames that arrive one at a time / in
                                      // pageable memory: [B x cap x 32 descriptors][B x cap x 12 points], or B packed frames;
                                      // allocated when first needed
    std::vector<int32_t> stagedNk;    // row counts of the frames push_async has staged
    int cursor = 0;                   // ps_vo_stream_pop: next pair of the held view
    bool haveView = false;            // pop_many has handed out a block that has not been released yet
    PsHostPairResults view{};
    long long diagLaunches = 0;       // launches attempted since configure (fault injection of -DPS_STREAM_DIAG builds counts these)
    double dbgT[3] = {0, 0, 0};       // PUTSLAM_HIP_STREAM_DEBUG=1: host seconds inside the uploads' / the batched call's /
    long long dbgN = 0;               // the downloads' submission, printed when the pipeline is released
    AsyncRing ring;
    AsyncMini mini;
};

namespace {

using psdev::CopySegs;
using psdev::MiniMeta;
using psdev::ps_copy_segments;
using psdev::ps_mini_copy_in;
using psdev::ps_pack_results_to_host;
using psledger::Chunk;
using psledger::ResLayout;

int async_fail(PsVoStream *s, int code, const char *what, hipError_t e = hipSuccess) { return fail(s->ctx, code, what, e); }

double async_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

void async_free(PsVoAsync *a)
{
    if (a->ring.copyStream) (void)hipStreamSynchronize(a->ring.copyStream); // drain: uploads, lanes, downloads
    for (PsContext *c : a->laneCtx)
        if (c) (void)hipStreamSynchronize(c->stream);
    if (a->ring.copyOutStream) (void)hipStreamSynchronize(a->ring.copyOutStream);
    if (a->dbgN > 0 && std::getenv("PUTSLAM_HIP_STREAM_DEBUG"))
        fprintf(stderr, "[ps stream] %lld chunks of <= %d frames on %d lanes (+ %d ahead): host us per chunk: upload %.1f, batched call %.1f, download %.1f\n",
                a->dbgN, a->led.B, a->led.lanes, a->led.ahead, 1e6 * a->dbgT[0] / a->dbgN, 1e6 * a->dbgT[1] / a->dbgN, 1e6 * a->dbgT[2] / a->dbgN);
    for (AsyncLane &l : a->lane) {
        release(l.meta);
        release(l.res);
        if (l.hmeta) (void)hipHostFree(l.hmeta);
        if (l.hres) (void)hipHostFree(l.hres);
        if (l.evDone) (void)hipEventDestroy(l.evDone);
        if (l.evRun) (void)hipEventDestroy(l.evRun);
        release(l.frames);
        if (l.gexec) (void)hipGraphExecDestroy(l.gexec);
    }
    for (PsContext *c : a->laneCtx)
        if (c) ps_context_destroy(c);
    for (uint8_t *h : a->stagePool)
        if (h) (void)hipHostFree(h);
    for (hipEvent_t e : a->ring.upEv)
        if (e) (void)hipEventDestroy(e);
    release(a->ring.desc);
    release(a->ring.pts);
    if (a->ring.spareHres) (void)hipHostFree(a->ring.spareHres);
    if (a->ring.heldHres) (void)hipHostFree(a->ring.heldHres);
    if (a->ring.copyStream) (void)hipStreamDestroy(a->ring.copyStream);
    if (a->ring.copyOutStream) (void)hipStreamDestroy(a->ring.copyOutStream);
    if (a->mini.loneHost) (void)hipHostFree(a->mini.loneHost);
    if (a->mini.loneReadEv) (void)hipEventDestroy(a->mini.loneReadEv);
    delete a;
}

bool is_pinned_host(const void *p)
{
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError(); // pageable memory: "invalid value", not an error of ours
        return false;
    }
    return at.type == hipMemoryTypeHost;
}

// frames on the device as the batched call takes them: two arrays, or (pts null) packed frames of the stream's stride
PsFrameSet frame_set(const PsVoStream *s, const void *desc, const void *pts, const int32_t *nk, int frames)
{
    PsFrameSet fs;
    fs.desc = (const uint8_t *)desc;
    fs.pts = (const float *)(pts ? pts : (const uint8_t *)desc + (size_t)s->cap * 32);
    fs.nkpts = nk;
    fs.numFrames = frames;
    fs.maxKpts = s->cap;
    fs.descFrameStride = fs.ptsFrameStride = pts ? 0 : s->async->packStride;
    return fs;
}

// inliers / poses only: a kernel writes just those of P pairs from the device block into the mapped pinned one
void launch_pack_results(const ResLayout &res, hipStream_t stream, int P, int mode, uint8_t *dres, uint8_t *hresDev)
{
    const PsPairResults d = res.device(dres), h = res.device(hresDev);
    hipLaunchKernelGGL(ps_pack_results_to_host, dim3((unsigned)P), dim3(kBlock), 0, stream, (const PsDMatch *)d.matches,
                       (const int32_t *)d.numMatches, (const uint8_t *)d.inlierMask, (const float *)d.pose, (const PsRansacStats *)d.stats,
                       (int)res.cap, mode, h.matches, h.pose, h.stats, h.numMatches);
}

// A chunk's frames as a submit takes them: host pointers for the ring's uploads (packed: `desc` alone), and for a mini chunk the
// device view its copy-in kernel reads them through.  inPlace: they lie in the caller's pinned memory, not in a staging area.
struct ChunkFrames {
    const uint8_t *desc = nullptr;
    const float *pts = nullptr;
    const uint8_t *dev = nullptr;
    bool inPlace = false;
};

// the pinned staging area of the chunk that will be submitted next (Ledger::next_area: written again only when every chunk
// that read it has been popped)
int stage_area(PsVoStream *s, ChunkFrames *out)
{
    PsVoAsync *a = s->async;
    PsContext *ctx = s->ctx;
    const size_t k = (size_t)a->led.next_area(), cap = (size_t)s->cap;
    uint8_t *&h = a->stagePool[k];
    if (!h) {
        PS_HIP(hipHostMalloc((void **)&h, a->packed ? (size_t)a->led.B * a->packStride : (size_t)a->led.B * cap * 44, hipHostMallocDefault));
        if (a->led.mini) PS_HIP(hipHostGetDevicePointer((void **)&a->mini.stagePoolDev[k], h, 0));
    }
    *out = ChunkFrames{h, a->packed ? nullptr : reinterpret_cast<const float *>(h + (size_t)a->led.B * cap * 32),
                       a->led.mini ? a->mini.stagePoolDev[k] : nullptr, false};
    return PS_OK;
}

// n rows of one frame (descriptors `descStep` bytes apart) into slot k of a staging area, in the stream's layout
void stage_frame(const PsVoStream *s, const ChunkFrames &area, int k, const uint8_t *desc, size_t descStep, const void *pts, int n)
{
    const PsVoAsync *a = s->async;
    const size_t cap = (size_t)s->cap;
    uint8_t *h = const_cast<uint8_t *>(area.desc);
    uint8_t *hd = h + (size_t)k * (a->packed ? a->packStride : cap * 32);
    uint8_t *hp = a->packed ? hd + cap * 32 : h + (size_t)a->led.B * cap * 32 + (size_t)k * cap * 12;
    if (n <= 0) return;
    if (descStep == PS_DESC_BYTES) {
        memcpy(hd, desc, (size_t)n * 32);
    } else {
        for (int i = 0; i < n; ++i) memcpy(hd + (size_t)i * 32, desc + (size_t)i * descStep, 32);
    }
    memcpy(hp, pts, (size_t)n * 12);
}

// ---- a chunk's launch: begin, the form's own launches, commit ----

// The chunk the next n frames make, on the place and lane the ledger gives it.  Nothing is taken yet: a chunk that cannot be
// queued completely leaves the ledger as it found it (async_abort_chunk does the rest).
int chunk_begin(PsVoStream *s, const Chunk &c)
{
    PsVoAsync *a = s->async;
    a->lane[(size_t)c.place].ctx = a->laneCtx[(size_t)c.lane];
    a->diagLaunches++;
#ifdef PS_STREAM_DIAG
    // fault injection (tests/test_gpu_stream_async.py builds the library with -DPS_STREAM_DIAG; the shipped one does not contain
    // this): the N-th chunk since configure fails before it has queued anything / behind its launches (chunk_commit)
    static const char *diagFail = std::getenv("PUTSLAM_HIP_STREAM_DIAG_FAIL_CHUNK");
    if (diagFail && std::atoll(diagFail) == a->diagLaunches - 1) return async_fail(s, PS_ERR_HIP, "pipelined chunk: injected failure (PS_STREAM_DIAG)");
#endif
    return PS_OK;
}

// The chunk's launches are queued on `stream`: evDone (and `alsoBehind`) behind them, and the chunk takes its place.
int chunk_commit(PsVoStream *s, const Chunk &c, AsyncLane &l, hipStream_t stream, hipEvent_t alsoBehind = nullptr)
{
    PsVoAsync *a = s->async;
    PsContext *ctx = s->ctx;
#ifdef PS_STREAM_DIAG
    static const char *diagFailAfter = std::getenv("PUTSLAM_HIP_STREAM_DIAG_FAIL_AFTER");
    if (diagFailAfter && std::atoll(diagFailAfter) == a->diagLaunches - 1)
        return fail(ctx, PS_ERR_HIP, "pipelined chunk: injected failure behind the batched call (PS_STREAM_DIAG)");
#endif
    PS_HIP(hipEventRecord(l.evDone, stream));
    if (alsoBehind) PS_HIP(hipEventRecord(alsoBehind, stream));
    a->led.commit(c);
    a->dbgN++;
    return PS_OK;
}

// (experiment of -DPS_STREAM_DIAG builds, results meaningless: PUTSLAM_HIP_STREAM_DIAG_NO_UPLOAD=1 skips the frames' way to the
// device after the first 64 chunks -- the chunks then run on whatever frames the device holds; it told what the pipeline does when
// the link costs nothing, profiles/r05h/stream_limits.txt.  The shipped library does not contain it.)
bool diag_no_upload(const PsVoAsync *a)
{
    bool skip = false;
#ifdef PS_STREAM_DIAG
    static const bool diagNoUpload = std::getenv("PUTSLAM_HIP_STREAM_DIAG_NO_UPLOAD") != nullptr;
    skip = diagNoUpload && a->led.chunkSeq >= 64;
#endif
    (void)a;
    return skip;
}

int chunk_failed(PsVoStream *s, PsContext *lc, int rc)
{
    s->ctx->err = std::string("pipelined chunk: ") + lc->err;
    return rc;
}

// One chunk of the ring form: n frames (pinned host memory: desc n x cap x 32, pts n x cap x 3, or n packed frames; row counts
// nk) -> ring -> the next place, launched on the next lane's stream: meta block, the batched call's launches behind the
// chunk's uploads, the download.  The caller has checked the ledger's room().
int ring_submit_body(PsVoStream *s, const ChunkFrames &fr, const int32_t *nk, int n)
{
    PsVoAsync *a = s->async;
    AsyncRing &r = a->ring;
    PsContext *ctx = s->ctx;
    const size_t cap = (size_t)s->cap;
    const Chunk c = a->led.next(n);
    const double t0 = async_now();
    hipEvent_t up = r.upEv[(size_t)c.area];
    if (!diag_no_upload(a)) {
        // (packed: `desc` = the chunk's packed frames: ONE transfer, no idle link between a descriptor and a point upload)
        const size_t step = a->packed ? a->packStride : cap * 32;
        PS_HIP(hipMemcpyAsync((uint8_t *)r.desc.p + (size_t)c.pos0 * step, fr.desc, (size_t)n * step, hipMemcpyHostToDevice, r.copyStream));
        if (!a->packed)
            PS_HIP(hipMemcpyAsync((uint8_t *)r.pts.p + (size_t)c.pos0 * cap * 12, fr.pts, (size_t)n * cap * 12, hipMemcpyHostToDevice, r.copyStream));
    }
    PS_HIP(hipEventRecord(up, r.copyStream));
    // (the slots are this chunk's to write: no chunk alive reads them, whether this one is committed or not)
    for (int i = 0; i < n; ++i) r.nk[(size_t)(c.pos0 + i)] = nk[i];
    a->dbgT[0] += async_now() - t0;
    const int P = c.pairs();
    if (P <= 0) {
        // a lone first frame: nothing to run, no place taken; its staging area (if it came through one) is reused by the
        // next push, so the upload is waited for here
        PS_HIP(hipStreamSynchronize(r.copyStream));
        a->led.lone_first_frame(c);
        return PS_OK;
    }
    // consecutive chunks on consecutive lanes; a lane's stream orders the chunks it is given (its scratch arena is theirs in turn)
    int rc = chunk_begin(s, c);
    if (rc != PS_OK) return rc;
    AsyncLane &l = a->lane[(size_t)c.place];
    PsContext *lc = l.ctx;
    const double t1 = async_now();
    int32_t *pm = l.hmeta;
    c.pair_list(pm);
    // (a snapshot of the ring's row counts as they are NOW: it may already hold those of later chunks, never other values for
    // the slots this chunk reads -- those are not written again while it is alive)
    memcpy(pm + 2 * (size_t)a->led.B, r.nk.data(), (size_t)a->led.ringFrames * sizeof(int32_t));
    CopySegs meta{};
    meta.src[0] = l.hmetaDev;
    meta.dst[0] = l.meta.p;
    meta.bytes[0] = ((unsigned long long)2 * a->led.B + a->led.ringFrames) * sizeof(int32_t);
    meta.n = 1;
    hipLaunchKernelGGL(ps_copy_segments, dim3(1), dim3(256), 0, lc->stream, meta); // (a few KB: beside the previous chunk's kernels)
    PS_HIP(hipGetLastError());
#ifdef PS_STREAM_DIAG
    // (experiment, results meaningless: the chunk's kernels do not wait for its upload -- what the upload -> lane dependency costs)
    static const bool diagNoUpWait = std::getenv("PUTSLAM_HIP_STREAM_DIAG_NO_UPWAIT") != nullptr;
    if (!diagNoUpWait)
#endif
    PS_HIP(hipStreamWaitEvent(lc->stream, up, 0));
    const PsFrameSet fs = frame_set(s, r.desc.p, a->packed ? nullptr : r.pts.p, (const int32_t *)l.meta.p + 2 * (size_t)a->led.B, a->led.ringFrames);
    uint8_t *dres = (uint8_t *)l.res.p;
    PsPairResults out = a->res.device(dres);
    PsRansacConfig c2 = a->cfg;
    c2.seed = a->cfg.seed + (uint64_t)c.firstPair;
    rc = ps_vo_pairs_device(lc, &a->prm, &c2, a->haveK ? a->K : nullptr, &fs, (const int32_t *)l.meta.p, P, &out);
    if (rc != PS_OK) return chunk_failed(s, lc, rc);
    const double t2 = async_now();
    // The download goes out on a stream of its own, behind an event, when the process has hardware queues to spare (async_build):
    // this runtime executes a device -> host hipMemcpyAsync as a blit kernel whatever stream it is queued on
    // (profiles/r05e/timeline_tail.txt), and on the lane's own stream that kernel sat between the lane's launches (29 % of the
    // time one was running, profiles/r05d); on the copy-out stream it overlaps the lane's NEXT chunk instead: + 11 ... 18 % with
    // six lanes.
    hipStream_t ds = r.downloadsOnLane ? lc->stream : r.copyOutStream;
    if (!r.downloadsOnLane) {
        PS_HIP(hipEventRecord(l.evRun, lc->stream));
        PS_HIP(hipStreamWaitEvent(ds, l.evRun, 0));
    }
    if (a->resultMode != PS_RESULTS_FULL) {
        // behind kernel 4 (on the download stream too: on the lane's own stream the lane's next chunk waited behind its writes
        // over the link)
        launch_pack_results(a->res, ds, P, a->resultMode, dres, l.hresDev);
        PS_HIP(hipGetLastError());
    } else if (P == a->led.B) {
        PS_HIP(hipMemcpyAsync(l.hres, dres, a->res.bytes, hipMemcpyDeviceToHost, ds));
    } else {
        ResLayout::Seg seg[5];
        a->res.segments((size_t)P, 1, seg);
        for (int k = 0; k < 5; ++k) PS_HIP(hipMemcpyAsync(l.hres + seg[k].off, dres + seg[k].off, seg[k].bytes, hipMemcpyDeviceToHost, ds));
    }
    rc = chunk_commit(s, c, l, ds);
    if (rc != PS_OK) return rc;
    const double t3 = async_now();
    if (const char *v = std::getenv("PUTSLAM_HIP_STREAM_DEBUG"))
        if (v[0] == '2')
            fprintf(stderr, "[chunk at pair %lld lane %d P %d] call %.1f download %.1f\n", c.firstPair, c.place, P, 1e6 * (t2 - t1),
                    1e6 * (t3 - t2));
    a->dbgT[1] += t2 - t1;
    a->dbgT[2] += t3 - t2;
    return PS_OK;
}

// The launches of one mini chunk on its lane's stream: frames in, kernels 1 - 4, results out (what a place's graph holds).
int mini_enqueue(PsVoStream *s, AsyncLane &l, PsContext *lc, const Plan &pl, int P)
{
    PsVoAsync *a = s->async;
    PsContext *ctx = s->ctx;
    MiniMeta *dm = (MiniMeta *)l.meta.p;
    const int groups = 8;
    if (diag_no_upload(a)) { // (the meta block alone travels)
        CopySegs up{};
        up.src[0] = l.hmetaDev;
        up.dst[0] = dm;
        up.bytes[0] = sizeof(MiniMeta);
        up.n = 1;
        hipLaunchKernelGGL(ps_copy_segments, dim3(1), dim3(64), 0, lc->stream, up);
    } else
        hipLaunchKernelGGL(ps_mini_copy_in, dim3((unsigned)((a->led.B + 1) * groups)), dim3(256), 0, lc->stream, (const MiniMeta *)l.hmetaDev, dm,
                           (uint8_t *)l.frames.p, s->cap, (unsigned long long)a->packStride, groups);
    PS_HIP(hipGetLastError());
    const PsFrameSet fs = frame_set(s, l.frames.p, nullptr, dm->nk, a->led.B + 1);
    uint8_t *dres = (uint8_t *)l.res.p;
    const PsPairResults out = a->res.device(dres);
    int rc = run_match_stage(lc, fs, dm->pairs, P, &pl, out.matches, out.numMatches, 0);
    if (rc == PS_OK) rc = run_ransac_stage(lc, pl, P, s->cap, out.matches, out.numMatches, s->cap, out.pose, out.inlierMask, out.stats, 2);
    if (rc != PS_OK) return chunk_failed(s, lc, rc);
    if (a->resultMode != PS_RESULTS_FULL) {
        launch_pack_results(a->res, lc->stream, P, a->resultMode, dres, l.hresDev);
    } else {
        ResLayout::Seg seg[5];
        a->res.segments((size_t)P, 4, seg);
        CopySegs down{};
        for (int k = 0; k < 5; ++k) {
            down.src[k] = dres + seg[k].off;
            down.dst[k] = l.hresDev + seg[k].off;
            down.bytes[k] = seg[k].bytes;
        }
        down.n = 5;
        const unsigned groupsOut = (unsigned)((seg[0].bytes / 16 + 255) / 256);
        hipLaunchKernelGGL(ps_copy_segments, dim3(groupsOut < 1 ? 1 : (groupsOut > 32 ? 32 : groupsOut)), dim3(256), 0, lc->stream, down);
    }
    PS_HIP(hipGetLastError());
    return PS_OK;
}

// the plan of a mini chunk of P pairs on lane lc: the seed is read from the place's meta block
int mini_plan(PsVoStream *s, AsyncLane &l, PsContext *lc, int P, Plan &pl)
{
    PsVoAsync *a = s->async;
    int rc = make_plan(lc, &a->prm, &a->cfg, a->haveK ? a->K : nullptr, s->cap, s->cap, pl);
    if (rc == PS_OK) {
        pl.ma.seedDev = reinterpret_cast<const uint64_t *>(&((MiniMeta *)l.meta.p)->seed);
        rc = prepare_score(lc, pl, P, s->cap);
    }
    return rc == PS_OK ? PS_OK : chunk_failed(s, lc, rc);
}

// the place's full chunk as a graph, once an un-captured full chunk has sized its lane's arena (no graph and no error: capture
// is not available here, ordinary launches from now on)
int mini_capture(PsVoStream *s, AsyncLane &l, PsContext *lc, int laneIdx, int P)
{
    PsVoAsync *a = s->async;
    PsContext *ctx = s->ctx;
    Plan pl;
    int rc = mini_plan(s, l, lc, P, pl);
    if (rc != PS_OK) return rc;
    PS_ENSURE(lc->keys, (size_t)P * s->cap * sizeof(uint32_t));
    rc = keys_clean(lc, (size_t)P * s->cap * sizeof(uint32_t)); // (outside the capture: a replay finds the block as its capture did)
    if (rc != PS_OK) return chunk_failed(s, lc, rc);
    if (lc->arenaGen != a->mini.laneWarmGen[(size_t)laneIdx]) return PS_OK;
    hipGraph_t graph = nullptr;
    if (hipStreamBeginCapture(lc->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
        const int r = mini_enqueue(s, l, lc, pl, P);
        const hipError_t e2 = hipStreamEndCapture(lc->stream, &graph);
        if (r == PS_OK && e2 == hipSuccess && graph && hipGraphInstantiate(&l.gexec, graph, nullptr, nullptr, 0) != hipSuccess) l.gexec = nullptr;
        if (r != PS_OK || e2 != hipSuccess) l.gexec = nullptr;
        if (graph) (void)hipGraphDestroy(graph);
    }
    if (!l.gexec) {
        s->graphsEnabled = false;
        (void)hipGetLastError();
        ctx->err.clear();
    } else {
        l.gexecGen = lc->arenaGen;
    }
    return PS_OK;
}

// One mini chunk: n frames (fr.desc on the host, fr.dev as the copy-in kernel sees them: a staging area, or pinned packed
// frames of the caller's, read in place) -> the next place, on that place's lane.  The caller has checked the ledger's room().
int mini_submit_body(PsVoStream *s, const ChunkFrames &fr, const int32_t *nk, int n)
{
    PsVoAsync *a = s->async;
    AsyncMini &m = a->mini;
    PsContext *ctx = s->ctx;
    const Chunk c = a->led.next(n);
    const int P = c.pairs();
    if (P <= 0) {
        // A lone first frame (the stream's first, or the first after a reset): nothing to run, no place taken -- and therefore no
        // staging area either (the ledger's reuse invariant).  The frame stays where the caller keeps it, or moves to a buffer
        // of its own; that buffer is written again only after the chunk that read it has finished.
        if (!fr.inPlace) {
            if (!m.loneHost) {
                PS_HIP(hipHostMalloc((void **)&m.loneHost, a->packStride, hipHostMallocDefault));
                PS_HIP(hipHostGetDevicePointer((void **)&m.loneDev, m.loneHost, 0));
                PS_HIP(hipEventCreateWithFlags(&m.loneReadEv, hipEventDisableTiming));
            }
            if (m.loneReadPending) {
                PS_HIP(hipEventSynchronize(m.loneReadEv));
                m.loneReadPending = false;
            }
            stage_frame(s, ChunkFrames{m.loneHost}, 0, fr.desc, PS_DESC_BYTES, fr.desc + (size_t)s->cap * 32, nk[0]);
        }
        // (the caller's pinned memory: untouched until the pair it is the previous frame of has been popped)
        m.haloDev = fr.inPlace ? fr.dev : m.loneDev;
        m.haloIsLone = !fr.inPlace;
        m.haloNk = nk[0];
        a->led.lone_first_frame(c);
        return PS_OK;
    }
    int rc = chunk_begin(s, c);
    if (rc != PS_OK) return rc;
    AsyncLane &l = a->lane[(size_t)c.place];
    PsContext *lc = l.ctx;
    MiniMeta *hm = (MiniMeta *)l.hmeta;
    memset(hm, 0, sizeof *hm);
    c.pair_list(hm->pairs);
    hm->nk[0] = c.first ? 0 : m.haloNk;
    for (int i = 0; i < n; ++i) hm->nk[1 + i] = nk[i];
    hm->n = n;
    hm->first = c.first;
    hm->seed = a->cfg.seed + (uint64_t)c.firstPair;
    hm->src[0] = c.first ? nullptr : m.haloDev;
    for (int i = 0; i < n; ++i) hm->src[1 + i] = fr.dev + (size_t)i * a->packStride;
    const bool full = P == a->led.B && !c.first;
    bool launched = false;
    if (full && m.graphs && s->graphsEnabled) { // (PUTSLAM_HIP_STREAM_GRAPH=1; PUTSLAM_HIP_NO_GRAPH=1 at ps_vo_stream_create wins)
        if (l.gexec && l.gexecGen != lc->arenaGen) { // the lane's arena has moved since the capture
            (void)hipGraphExecDestroy(l.gexec);
            l.gexec = nullptr;
        }
        if (!l.gexec && m.laneWarmGen[(size_t)c.lane] == lc->arenaGen && lc->arenaGen != 0) {
            rc = mini_capture(s, l, lc, c.lane, P);
            if (rc != PS_OK) return rc;
        }
        if (l.gexec) {
            PS_HIP(hipGraphLaunch(l.gexec, lc->stream));
            m.graphLaunches++;
            launched = true;
        }
    }
    if (!launched) {
        // the plan of a full chunk is made once per place (parameters, P and the lane's arena do not change between chunks): the
        // host side of a chunk is its staging copy and seven launches
        const bool cached = full && l.planGen != 0 && l.planGen == lc->arenaGen;
        Plan local;
        Plan &pl = full ? l.plan : local;
        if (!cached) {
            l.planGen = 0;
            rc = mini_plan(s, l, lc, P, pl);
            if (rc != PS_OK) return rc;
        }
        rc = mini_enqueue(s, l, lc, pl, P);
        if (rc != PS_OK) return rc;
        if (full) {
            m.laneWarmGen[(size_t)c.lane] = lc->arenaGen;
            l.planGen = lc->arenaGen; // (the plan points at the blocks prepare_score sized -- counts, parked models, stop tables --;
                                      // the launches above only grow OTHER blocks, so the plan stays good for the arena as it is now)
        }
    }
    // (a chunk that read the lone-frame buffer as its previous frame: the buffer is free again behind it)
    const bool readLone = m.haloIsLone && !c.first;
    rc = chunk_commit(s, c, l, lc->stream, readLone ? m.loneReadEv : nullptr);
    if (rc != PS_OK) return rc;
    if (readLone) m.loneReadPending = true;
    // the stream's latest frame from now on: the next chunk reads it from this staging slot -- or from the caller's pinned block
    m.haloDev = fr.dev + (size_t)(n - 1) * a->packStride;
    m.haloNk = nk[n - 1];
    m.haloIsLone = false;
    return PS_OK;
}

// A chunk could not be queued (an allocation or a HIP call failed somewhere between its upload and its download).  Whatever
// part of it WAS queued is drained -- nothing is in flight on a place that is still marked free --, the chunk's frames are
// dropped as a unit, and the stream continues as after ps_vo_stream_reset: the next frame has no predecessor, pair numbering
// restarts at 0, the epoch advances (include/putslam_hip.h).  Chunks submitted before keep their place, numbering and epoch.
int async_abort_chunk(PsVoStream *s, int rc)
{
    PsVoAsync *a = s->async;
    const std::string why = s->ctx->err;
    if (a->ring.copyStream) (void)hipStreamSynchronize(a->ring.copyStream);
    PsContext *lc = a->laneCtx.empty() ? nullptr : a->laneCtx[(size_t)a->led.next_lane()];
    if (lc) (void)hipStreamSynchronize(lc->stream);
    a->mini.haloDev = nullptr;
    a->mini.haloIsLone = false;
    if (a->ring.copyOutStream) (void)hipStreamSynchronize(a->ring.copyOutStream);
    (void)hipGetLastError();
    a->led.abort();
    s->ctx->err = why + " -- pipelined stream: the chunk's frames were dropped; the next frame starts a new epoch (pair numbering from 0)";
    return rc;
}

int async_submit(PsVoStream *s, const ChunkFrames &fr, const int32_t *nk, int n)
{
    const int rc = s->async->led.mini ? mini_submit_body(s, fr, nk, n) : ring_submit_body(s, fr, nk, n);
    return rc == PS_OK ? PS_OK : async_abort_chunk(s, rc);
}

// the frames push_async has collected, as a chunk (its place was reserved when the first of them was taken)
int async_submit_staged(PsVoStream *s)
{
    PsVoAsync *a = s->async;
    if (a->led.staged == 0) return PS_OK;
    ChunkFrames area; // (the one push_async has been filling: the next chunk's)
    int rc = stage_area(s, &area);
    if (rc) return rc;
    const int n = a->led.take_staged();
    return async_submit(s, area, a->stagedNk.data(), n);
}

// ---- one push path ----

// Frames as a push call names them: base pointers and per-frame strides of the descriptors and the points, row counts.
struct FrameSource {
    const uint8_t *desc, *pts;
    size_t descStride, ptsStride;
    const int32_t *nk;
    int frames;
};

// What a push reads in place -- pinned memory, which the caller leaves untouched until the results of its frames (for a chunk's
// last frame: of the NEXT pair, which reads it as its previous frame) have been popped -- and not through a staging area:
//   ring, two arrays                  both pointers pinned (uploaded from there)
//   ring, packed, fed two arrays      never (the frames are packed on their way through the staging area)
//   ring, packed, fed packed          pinned
//   mini                              pinned, packed, contiguous, and a device view of it exists (*dev): the copy-in kernel reads
//                                     it (88 KB less for the host to copy per 2000-keypoint frame)
bool reads_in_place(const PsVoStream *s, const FrameSource &src, const uint8_t **dev)
{
    const PsVoAsync *a = s->async;
    const bool fedPacked = src.descStride == a->packStride && src.pts == src.desc + (size_t)s->cap * 32;
    *dev = nullptr;
    if (!a->packed) return is_pinned_host(src.desc) && is_pinned_host(src.pts);
    if (!fedPacked || !is_pinned_host(src.desc)) return false;
    if (!a->led.mini) return true;
    if (hipHostGetDevicePointer((void **)dev, const_cast<uint8_t *>(src.desc), 0) == hipSuccess && *dev) return true;
    (void)hipGetLastError();
    *dev = nullptr;
    return false;
}

// Several frames into the stream (push_many / push_many_packed): frames staged by push_async before go first, as a chunk of
// their own; these follow in chunks of at most chunkFrames, the last one included -- everything is submitted when the call
// returns.  All or nothing: a place for every one of those chunks.
int push_frames(PsVoStream *s, const FrameSource &src, const char *who)
{
    PsVoAsync *a = s->async;
    auto refuse = [&](int code, const char *why) { return async_fail(s, code, (std::string(who) + why).c_str()); }; // (no string on the way through)
    for (int i = 0; i < src.frames; ++i)
        if (src.nk[i] < 0 || src.nk[i] > s->cap) return refuse(PS_ERR_BAD_ARG, ": row count out of range");
    if (src.frames == 0) return PS_OK;
    if (a->led.chunks_for(src.frames) > a->led.room()) return refuse(PS_ERR_BUSY, ": not enough room for these frames (pop results first, or push fewer)");
    int rc = async_submit_staged(s);
    if (rc) return rc;
    const uint8_t *dev = nullptr;
    const bool inPlace = reads_in_place(s, src, &dev);
    for (int f0 = 0; f0 < src.frames; f0 += a->led.B) {
        const int n = src.frames - f0 < a->led.B ? src.frames - f0 : a->led.B;
        ChunkFrames fr;
        if (inPlace) {
            fr = ChunkFrames{src.desc + (size_t)f0 * src.descStride, reinterpret_cast<const float *>(src.pts + (size_t)f0 * src.ptsStride),
                             dev ? dev + (size_t)f0 * a->packStride : nullptr, true};
        } else { // pageable frames, or another layout than the stream's: through the chunk's pinned staging area, frame by frame
            rc = stage_area(s, &fr);
            if (rc) return rc;
            for (int i = 0; i < n; ++i)
                stage_frame(s, fr, i, src.desc + (size_t)(f0 + i) * src.descStride, PS_DESC_BYTES, src.pts + (size_t)(f0 + i) * src.ptsStride,
                            src.nk[f0 + i]);
        }
        rc = async_submit(s, fr, src.nk + f0, n);
        if (rc) return rc;
    }
    return PS_OK;
}

// device / pinned blocks, streams, events and lane contexts of a freshly configured pipeline
int async_build(PsVoStream *s, int chunkFrames, int lanes, int ahead)
{
    PsVoAsync *a = s->async;
    AsyncRing &r = a->ring;
    PsContext *ctx = s->ctx;
    const size_t cap = (size_t)s->cap, B = (size_t)chunkFrames;
    // small chunks as one graph per place (AsyncMini); PUTSLAM_HIP_STREAM_MINI=0 keeps round 5's form for them (A/B, tests)
    const char *m = std::getenv("PUTSLAM_HIP_STREAM_MINI");
    a->led.configure(chunkFrames, lanes, ahead, chunkFrames <= psdev::kMiniFrames && !(m && std::atoi(m) == 0));
    const char *g = std::getenv("PUTSLAM_HIP_STREAM_GRAPH");
    a->mini.graphs = g && std::atoi(g) != 0;
    a->res = ResLayout(B, cap);
    a->stagedNk.assign(B, 0);
    a->stagePool.assign((size_t)a->led.areas(), nullptr);
    a->packed = a->led.mini || s->asyncFrameLayout == PS_FRAMES_PACKED;
    a->packStride = (cap * 44 + 15) & ~(size_t)15;
    if (a->led.mini) {
        a->mini.laneWarmGen.assign((size_t)lanes, 0);
        a->mini.stagePoolDev.assign(a->stagePool.size(), nullptr);
        a->mini.viewBuf.assign(a->res.alloc_bytes(), 0);
    } else {
        const size_t ringFrames = (size_t)a->led.ringFrames;
        r.nk.assign(ringFrames, 0);
        r.upEv.assign(a->stagePool.size(), nullptr);
        for (hipEvent_t &e : r.upEv) PS_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        PS_ENSURE(r.desc, a->packed ? ringFrames * a->packStride : ringFrames * cap * 32);
        if (!a->packed) PS_ENSURE(r.pts, ringFrames * cap * 12);
        PS_HIP(hipHostMalloc((void **)&r.spareHres, a->res.alloc_bytes(), hipHostMallocDefault));
        PS_HIP(hipHostGetDevicePointer((void **)&r.spareHresDev, r.spareHres, 0));
    }
    // (mini streams create the two copy streams too and leave them idle: the process's streams meet its hardware queues in the
    // order measured)
    PS_HIP(hipStreamCreateWithFlags(&r.copyStream, hipStreamNonBlocking));
    PS_HIP(hipStreamCreateWithFlags(&r.copyOutStream, hipStreamNonBlocking));
    // A stream of its own for the downloads pays only when it also gets a hardware queue of its own: with the runtime's
    // default of four queues (or eight shared with the host's other streams) it lands on a lane's or the upload stream's queue
    // and serialises with it -- 130 k instead of 390 k frame-pairs/s in bench.py's process (profiles/r05f/hw_queues.txt).  The
    // runtime has no query for the number of queues; the environment variable that sets it is read instead.
    {
        int queues = 4; // (ROCclr's default)
        if (const char *q = std::getenv("GPU_MAX_HW_QUEUES")) queues = std::atoi(q);
        r.downloadsOnLane = queues < lanes + 6;
    }
    if (const char *v = std::getenv("PUTSLAM_HIP_STREAM_DOWNLOADS_ON_LANE")) r.downloadsOnLane = std::atoi(v) != 0;
    a->laneCtx.assign((size_t)lanes, nullptr);
    for (PsContext *&c : a->laneCtx) {
        int rc = ps_context_create(ctx->device, &c);
        if (rc != PS_OK) {
            c = nullptr;
            return fail(ctx, rc, "ps_vo_stream_configure_async: lane context");
        }
        psi_copy_options(c, ctx); // the lanes run what the stream's context would
        // Chunks on different lanes overlap, so the staged scoring pays from smaller batches on (prepare_score) -- from chunks of
        // 48 frames on: below, a chunk's extra launches cost more than its abandoned evaluations save (chunks of 32 / 64 frames on
        // three lanes, E1 / fixed / H = 4096: complete 204 k / 251 k, staged 156 k / 301 k frame-pairs/s, profiles/r06u/stream_small_chunks.txt)
        // (the decision is the stream's own: below 48 frames per chunk the lanes run as lone contexts whatever the stream's context says)
        if (B < 48) c->sideBySide = 0;
        else if (lanes > 1 && c->sideBySide < lanes) c->sideBySide = lanes;
    }
    a->lane.resize((size_t)a->led.places());
    const size_t metaBytes = std::max(((size_t)2 * B + a->led.ringFrames) * sizeof(int32_t), sizeof(psdev::MiniMeta));
    for (AsyncLane &l : a->lane) {
        if (a->led.mini) PS_ENSURE(l.frames, (B + 1) * a->packStride);
        PS_ENSURE(l.meta, metaBytes);
        PS_ENSURE(l.res, a->res.alloc_bytes());
        PS_HIP(hipHostMalloc((void **)&l.hmeta, metaBytes, hipHostMallocDefault));
        PS_HIP(hipHostMalloc((void **)&l.hres, a->res.alloc_bytes(), hipHostMallocDefault));
        PS_HIP(hipHostGetDevicePointer((void **)&l.hmetaDev, l.hmeta, 0));
        PS_HIP(hipHostGetDevicePointer((void **)&l.hresDev, l.hres, 0));
        PS_HIP(hipEventCreateWithFlags(&l.evRun, hipEventDisableTiming));
        PS_HIP(hipEventCreateWithFlags(&l.evDone, hipEventDisableTiming));
    }
    return PS_OK;
}

void release_view(PsVoAsync *a)
{
    AsyncRing &r = a->ring;
    if (r.heldHres) { // the block goes back to being the spare one
        r.spareHres = r.heldHres;
        r.spareHresDev = r.heldHresDev;
        r.heldHres = r.heldHresDev = nullptr;
    }
    a->cursor = 0;
    a->haveView = false;
    memset(&a->view, 0, sizeof a->view);
}

// what every push call checks first: the stream, its device, that the pipeline is configured
int push_enter(PsVoStream *s, const char *who)
{
    if (!s) return PS_ERR_BAD_ARG;
    int rc = bind(s->ctx);
    if (rc) return rc;
    if (!s->async) return async_fail(s, PS_ERR_BAD_ARG, (std::string(who) + ": call ps_vo_stream_configure_async first").c_str());
    return PS_OK;
}

} // namespace

static void async_release(PsVoStream *s)
{
    if (!s || !s->async) return;
    if (s->ctx) (void)hipSetDevice(s->ctx->device);
    async_free(s->async);
    s->async = nullptr;
}

static int async_reset(PsVoStream *s)
{
    int rc = bind(s->ctx);
    if (rc) return rc;
    rc = async_submit_staged(s); // (its place was reserved when push_async took the chunk's first frame)
    if (rc) return rc;
    s->async->led.reset();
    return PS_OK;
}

extern "C" {

int ps_vo_stream_configure_async(PsVoStream *s, const PsRansacParams *params, const PsRansacConfig *cfg, const float *K,
                                 int chunkFrames, int lanes)
{
    if (!s) return PS_ERR_BAD_ARG;
    PsContext *ctx = s->ctx;
    int rc = bind(ctx);
    if (rc) return rc;
    if (!params || !cfg) return fail(ctx, PS_ERR_BAD_ARG, "ps_vo_stream_configure_async: null params/config");
    if (cfg->sampleIdx) return fail(ctx, PS_ERR_BAD_ARG, "explicit sample streams are not supported by the streaming calls");
    if (chunkFrames == 0) chunkFrames = 128;
    // Lanes and places by chunk size, measured (profiles/r06i/stream_lanes_places.txt; round 5 ran six places in all, as six or
    // three lanes): chunks of a hundred frames and more fill the chip by themselves and run best as TWO launch chains with ONE more
    // chunk queued behind them -- 417 / 504 / 550 k frame-pairs/s at 125 / 250 / 500 frames per chunk against 398 / 474 / 445 k
    // with six places -- the same finding as the batch queue's (whole batches to two chains in turn); chunks of 48 .. 95 frames two
    // lanes and four places; smaller ones three lanes and six places; one to four frames six lanes (AsyncMini).
    if (lanes == 0) lanes = chunkFrames >= 48 ? 2 : (chunkFrames > psdev::kMiniFrames ? 3 : 6);
    if (chunkFrames < 1 || chunkFrames > 1024 || lanes < 2 || lanes > 8)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_vo_stream_configure_async: chunkFrames 1..1024, lanes 2..8");
    {
        // the parameters are checked here, not at the first chunk: a plan on the stream's own context
        Plan pl;
        rc = make_plan(ctx, params, cfg, K, s->cap, s->cap, pl);
        if (rc) return rc;
    }
    if (s->async) { // re-configuration: drain, drop what has not been popped
        async_free(s->async);
        s->async = nullptr;
    }
    PsVoAsync *a = new PsVoAsync();
    s->async = a;
    a->prm = *params;
    a->cfg = *cfg;
    a->cfg.sampleIdx = nullptr;
    a->haveK = K != nullptr;
    if (K) memcpy(a->K, K, sizeof a->K);
    a->resultMode = s->asyncResultMode;
    rc = async_build(s, chunkFrames, lanes,
                     ctx->streamAhead >= 0 ? ctx->streamAhead : (chunkFrames >= 96 ? 1 : (chunkFrames >= 48 ? 2 : (lanes < 6 ? 6 - lanes : 0))));
    if (rc != PS_OK) { // (the error text stays in the stream's context)
        const std::string why = ctx->err;
        async_free(a);
        s->async = nullptr;
        ctx->err = why;
    }
    return rc;
}

int ps_vo_stream_set_result_mode(PsVoStream *s, int mode)
{
    if (!s) return PS_ERR_BAD_ARG;
    if (mode < PS_RESULTS_FULL || mode > PS_RESULTS_POSES) return async_fail(s, PS_ERR_BAD_ARG, "ps_vo_stream_set_result_mode: 0 (full), 1 (inliers) or 2 (poses)");
    s->asyncResultMode = mode;
    return PS_OK;
}

int ps_vo_stream_push_async(PsVoStream *s, const uint8_t *desc, size_t descStep, const float *pts, int n)
{
    int rc = push_enter(s, "ps_vo_stream_push_async");
    if (rc) return rc;
    PsVoAsync *a = s->async;
    if (n < 0 || n > s->cap || (n > 0 && (!desc || !pts)) || descStep < PS_DESC_BYTES)
        return async_fail(s, PS_ERR_BAD_ARG, "ps_vo_stream_push_async: bad argument");
    // (the first frame of a chunk reserves the chunk's place; the later ones ride on it)
    if (a->led.staged == 0 && a->led.room() < 1) return async_fail(s, PS_ERR_BUSY, "ps_vo_stream_push_async: no room (pop results first)");
    ChunkFrames area;
    rc = stage_area(s, &area);
    if (rc) return rc;
    stage_frame(s, area, a->led.staged, desc, descStep, pts, n);
    a->stagedNk[(size_t)a->led.staged] = n;
    if (a->led.stage_one() == a->led.B) return async_submit_staged(s);
    return PS_OK;
}

int ps_vo_stream_flush(PsVoStream *s)
{
    int rc = push_enter(s, "ps_vo_stream_flush");
    if (rc) return rc;
    return async_submit_staged(s); // (the partly filled chunk's place was reserved by its first frame)
}

int ps_vo_stream_push_many(PsVoStream *s, const uint8_t *desc, const float *pts, const int32_t *nkpts, int numFrames)
{
    int rc = push_enter(s, "ps_vo_stream_push_many");
    if (rc) return rc;
    if (numFrames < 0 || (numFrames > 0 && (!desc || !pts || !nkpts)))
        return async_fail(s, PS_ERR_BAD_ARG, "ps_vo_stream_push_many: bad argument");
    const size_t cap = (size_t)s->cap;
    return push_frames(s, FrameSource{desc, reinterpret_cast<const uint8_t *>(pts), cap * 32, cap * 12, nkpts, numFrames}, "ps_vo_stream_push_many");
}

int ps_vo_stream_set_frame_layout(PsVoStream *s, int layout)
{
    if (!s) return PS_ERR_BAD_ARG;
    if (layout != PS_FRAMES_TWO_ARRAYS && layout != PS_FRAMES_PACKED)
        return async_fail(s, PS_ERR_BAD_ARG, "ps_vo_stream_set_frame_layout: 0 (two arrays) or 1 (packed frames)");
    s->asyncFrameLayout = layout;
    return PS_OK;
}

size_t ps_vo_stream_packed_stride(const PsVoStream *s) { return s ? (((size_t)s->cap * 44 + 15) & ~(size_t)15) : 0; }

int ps_vo_stream_push_many_packed(PsVoStream *s, const uint8_t *frames, size_t frameStride, const int32_t *nkpts, int numFrames)
{
    int rc = push_enter(s, "ps_vo_stream_push_many_packed");
    if (rc) return rc;
    PsVoAsync *a = s->async;
    if (!a->packed)
        return async_fail(s, PS_ERR_BAD_ARG, "ps_vo_stream_push_many_packed: the stream was configured for two arrays (ps_vo_stream_set_frame_layout "
                                             "before ps_vo_stream_configure_async)");
    if (numFrames < 0 || (numFrames > 0 && (!frames || !nkpts)) || frameStride != a->packStride)
        return async_fail(s, PS_ERR_BAD_ARG, "ps_vo_stream_push_many_packed: bad argument (frameStride must be ps_vo_stream_packed_stride())");
    return push_frames(s, FrameSource{frames, frames + (size_t)s->cap * 32, a->packStride, a->packStride, nkpts, numFrames}, "ps_vo_stream_push_many_packed");
}

int ps_vo_stream_pop_many(PsVoStream *s, int wait, PsHostPairResults *out)
{
    if (!s) return PS_ERR_BAD_ARG;
    int rc = bind(s->ctx);
    if (rc) return rc;
    PsVoAsync *a = s->async;
    if (!a || !out) return async_fail(s, PS_ERR_BAD_ARG, "ps_vo_stream_pop_many: bad argument / stream not configured");
    release_view(a);
    memset(out, 0, sizeof *out);
    out->maxKpts = s->cap;
    if (a->led.inFlight == 0) return PS_OK;
    AsyncLane &l = a->lane[(size_t)a->led.head];
    if (wait) {
        hipError_t e = hipEventSynchronize(l.evDone);
        if (e != hipSuccess) return async_fail(s, PS_ERR_HIP, "hipEventSynchronize(l.evDone)", e);
    } else {
        hipError_t q = hipEventQuery(l.evDone);
        if (q == hipErrorNotReady) {
            (void)hipGetLastError();
            return PS_OK;
        }
        if (q != hipSuccess) return async_fail(s, PS_ERR_HIP, "hipEventQuery", q);
    }
    const psledger::Place done = a->led.pop();
    uint8_t *blk = l.hres;
    if (a->led.mini) {
        // a mini chunk's results are a few tens of KB: copied out, so that the place keeps its pinned block (its graph writes
        // there) and is free at once
        blk = a->mini.viewBuf.data();
        ResLayout::Seg seg[5];
        a->res.segments((size_t)done.pairs, 1, seg);
        for (int k = 0; k < 5; ++k) // (the matches unless poses only, the mask only with full results)
            if (k >= 2 || (k == 0 ? a->resultMode != PS_RESULTS_POSES : a->resultMode == PS_RESULTS_FULL))
                memcpy(blk + seg[k].off, l.hres + seg[k].off, seg[k].bytes);
    } else {
        // the lane's block becomes the held one, the spare one the lane's: the lane is free now
        AsyncRing &r = a->ring;
        r.heldHres = l.hres;
        r.heldHresDev = l.hresDev;
        l.hres = r.spareHres;
        l.hresDev = r.spareHresDev;
        r.spareHres = r.spareHresDev = nullptr;
    }
    a->res.host(blk, a->resultMode, out);
    out->firstPair = done.firstPair;
    out->count = done.pairs;
    out->epoch = done.epoch;
    a->view = *out;
    a->haveView = true;
    return PS_OK;
}

int ps_vo_stream_pop(PsVoStream *s, int wait, PsDMatch *matches, int *nmatches, uint8_t *inlierMask, float *pose,
                     PsRansacStats *stats)
{
    if (!s) return PS_ERR_BAD_ARG;
    PsVoAsync *a = s->async;
    if (!a || !nmatches || !pose) return async_fail(s, PS_ERR_BAD_ARG, "ps_vo_stream_pop: bad argument / stream not configured");
    *nmatches = -1;
    if (!a->haveView || a->cursor >= a->view.count) {
        PsHostPairResults v;
        // (a frame that waits in a partly filled chunk is not submitted by a pop: ps_vo_stream_flush does that)
        int rc = ps_vo_stream_pop_many(s, wait, &v);
        if (rc) return rc;
        if (v.count == 0) return PS_OK;
    }
    const PsHostPairResults &v = a->view;
    const size_t i = (size_t)a->cursor, cap = (size_t)s->cap;
    int nm = v.numMatches[i];
    if (a->resultMode == PS_RESULTS_INLIERS) nm = v.stats[i].numInliers; // the inlier matches only, as Matcher::match returns them
    if (a->resultMode == PS_RESULTS_POSES) nm = 0;
    // (checked before the cursor moves: a call refused for its arguments loses no pair)
    if (nm > 0 && (!matches || !inlierMask)) return async_fail(s, PS_ERR_BAD_ARG, "ps_vo_stream_pop: null output");
    a->cursor++;
    memcpy(pose, v.pose + i * 16, 16 * sizeof(float));
    if (stats) *stats = v.stats[i];
    if (nm > 0) {
        memcpy(matches, v.matches + i * cap, (size_t)nm * sizeof(PsDMatch));
        if (a->resultMode == PS_RESULTS_FULL)
            memcpy(inlierMask, v.inlierMask + i * cap, (size_t)nm);
        else
            memset(inlierMask, 1, (size_t)nm);
    }
    *nmatches = nm;
    return PS_OK;
}

int ps_vo_stream_pending(const PsVoStream *s)
{
    if (!s || !s->async) return PS_ERR_BAD_ARG;
    const PsVoAsync *a = s->async;
    return a->led.pending() + (a->haveView ? a->view.count - a->cursor : 0);
}

long long ps_vo_stream_graph_launches(const PsVoStream *s)
{
    if (!s) return PS_ERR_BAD_ARG;
    return s->graphLaunches + (s->async ? s->async->mini.graphLaunches : 0);
}

void *ps_host_alloc(size_t bytes)
{
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}

void ps_host_free(void *p)
{
    if (p) (void)hipHostFree(p);
}

} // extern "C"
