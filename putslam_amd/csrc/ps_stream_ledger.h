// ps_stream_ledger.h -- every integer the pipelined stream (ps_stream_async.h) keeps, and the only code that changes one.
// Plain C++, no HIP: tests/cpp/test_stream_ledger.cpp compiles it alone and drives it through random call sequences.
//
// The pipeline has `lanes + ahead` PLACES, taken and freed in ring order (head = oldest chunk in flight, tail = next to take),
// `lanes + ahead + 1` pinned staging AREAS with one upload event each, and -- in the ring form -- a ring of frame slots in HBM.
// A chunk is ALIVE from commit() to pop().  While alive it reads its own area (its upload; a mini chunk's copy-in kernel), the
// last frame of its predecessor (in the ring: slot prevPos; a mini chunk: in the predecessor's area) and its own ring slots.
//
// THE REUSE INVARIANT.  Areas and upload events rotate with the COMMITTED chunks: chunk k uses area k % (lanes + ahead + 1), and
// chunkSeq moves in commit() and nowhere else.  A chunk is accepted only while a place is free, so at most lanes + ahead - 1
// chunks are alive then: chunks k - (lanes + ahead) + 1 .. k - 1, whose own areas and predecessors' areas are those of chunks
// k - (lanes + ahead) .. k - 1 -- never that of chunk k - (lanes + ahead + 1), which is the one chunk k writes.  A frame that takes
// no place (a lone first frame) and a chunk that fails before commit() therefore leave the rotation where it was: either one
// advancing it moves the reuse one chunk closer to a chunk that is still alive (the stream fuzz of round 6 found the first, 17 of
// 15 000 configurations, profiles/r06l/stream_and_queue_fuzz.txt; the advisor of round 6 the second).
//
// The ring's slots follow the same rule.  Between the oldest slot a chunk alive reads and the cursor lie, per chunk alive, its
// own <= B slots and ONE more -- the lone first frame before it, if it follows a reset --, the latest frame if no chunk has read
// it yet, and at most one jump to slot 0, which skips fewer than B; the new chunk writes at most B.  With lanes + ahead - 1
// chunks alive that is (lanes + ahead + 1) x B + lanes + ahead - 1 slots at most, and the ring has (lanes + ahead + 2) x B +
// lanes + ahead.  What takes no place must not move the cursor for good, or resets could walk it into slots still read: a lone
// frame that a reset drops hands its slot back, and a chunk that fails leaves the cursor where it was.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "putslam_hip.h"

namespace psledger {

// The result block of a chunk of up to B pairs, on the device and in pinned memory alike:
// [matches B x cap x 16][mask B x cap][pose B x 64][stats B x 40][numMatches B x 4], every segment from a 64-byte boundary.
struct ResLayout {
    size_t cap = 0, offMask = 0, offPose = 0, offStats = 0, offNum = 0, bytes = 0;
    struct Seg { size_t off, bytes; };
    ResLayout(size_t B = 0, size_t cap_ = 0) : cap(cap_)
    {
        offMask = B * cap * sizeof(PsDMatch);
        offPose = offMask + ((B * cap + 63) & ~(size_t)63);
        offStats = offPose + B * 64;
        offNum = offStats + ((B * sizeof(PsRansacStats) + 63) & ~(size_t)63);
        bytes = offNum + B * sizeof(int32_t);
    }
    size_t alloc_bytes() const { return (bytes + 15) & ~(size_t)15; }
    PsPairResults device(uint8_t *base) const
    {
        // (matches, numMatches, inlierMask, pose, stats: five pointer types, so the order is checked by the compiler)
        return PsPairResults{(PsDMatch *)base, (int32_t *)(base + offNum), base + offMask, (float *)(base + offPose), (PsRansacStats *)(base + offStats)};
    }
    // (the compact result modes leave the segments they do not return unwritten: no pointer to those)
    void host(const uint8_t *base, int mode, PsHostPairResults *r) const
    {
        r->matches = mode == PS_RESULTS_POSES ? nullptr : (const PsDMatch *)base;
        r->inlierMask = mode == PS_RESULTS_FULL ? base + offMask : nullptr;
        r->resultMode = mode;
        r->pose = (const float *)(base + offPose);
        r->stats = (const PsRansacStats *)(base + offStats);
        r->numMatches = (const int32_t *)(base + offNum);
    }
    // the five segments of the first P pairs; the mask's length rounded up to `maskRound` bytes (4: ps_copy_segments moves dwords)
    void segments(size_t P, size_t maskRound, Seg seg[5]) const
    {
        seg[0] = {0, P * cap * sizeof(PsDMatch)};
        seg[1] = {offMask, (P * cap + maskRound - 1) / maskRound * maskRound};
        seg[2] = {offPose, P * 64};
        seg[3] = {offStats, P * sizeof(PsRansacStats)};
        seg[4] = {offNum, P * sizeof(int32_t)};
    }
};

struct Place {
    int state = 0; // 0 free, 1 chunk in flight
    long long firstPair = 0;
    int pairs = 0, epoch = 0;
};

// The chunk the next n frames would be: where it goes and what it reads.  Slots are the ring's; a mini chunk's are those of
// its place's private frame set [1 + B] (slot 0 = the frame before the chunk's first one).
struct Chunk {
    int place = 0, lane = 0;
    int area = 0;            // staging area and upload event
    int pos0 = 0, n = 0;     // slots [pos0, pos0 + n)
    int first = 0;           // 1: the chunk's first frame has no predecessor (the stream's first frame, or after a reset)
    int prevPos = -1;        // slot of the frame before the chunk's first one
    long long firstPair = 0; // index of its first pair in the stream (-> seed)
    int epoch = 0;
    int pairs() const { return n - first; }
    // pair i of the chunk's frames, i in [first, n): query = previous frame, train = current (matcher.cpp:470-471)
    int query(int i) const { return i == 0 ? prevPos : pos0 + i - 1; }
    int train(int i) const { return pos0 + i; }
    void pair_list(int32_t *out) const
    {
        for (int i = first; i < n; ++i) out[2 * (i - first)] = query(i), out[2 * (i - first) + 1] = train(i);
    }
};

struct Ledger {
    int B = 0, lanes = 0, ahead = 0, ringFrames = 0;
    bool mini = false;
    std::vector<Place> place;
    int head = 0, tail = 0, inFlight = 0;
    long long launchSeq = 0; // chunks committed so far (ring form: chunk k runs on lane k % lanes)
    long long chunkSeq = 0;  // the rotation of areas and upload events: see THE REUSE INVARIANT
    int ringPos = 0;         // slot the next frame goes to
    int prevPos = -1;        // slot of the stream's latest frame (-1: the next frame has no predecessor)
    bool loneLatest = false; // the latest frame is a lone first frame: no chunk has read its slot
    long long pairCounter = 0;
    int epoch = 0;
    int staged = 0; // frames collected in the next chunk's staging area

    void configure(int B_, int lanes_, int ahead_, bool mini_)
    {
        B = B_, lanes = lanes_, ahead = ahead_, mini = mini_;
        ringFrames = mini ? B + 1 : (lanes + ahead + 2) * B + lanes + ahead; // (see THE REUSE INVARIANT)
        place.assign((size_t)(lanes + ahead), Place());
    }

    int places() const { return (int)place.size(); }
    int areas() const { return lanes + ahead + 1; }
    // chunks that can be accepted now: the free places (free ones are contiguous from `tail`)
    int room() const { return places() - inFlight; }
    int next_area() const { return (int)(chunkSeq % areas()); }
    // (the mini form's lane is fixed per place: the place's graph holds its lane's arena pointers)
    int next_lane() const { return (int)((mini ? (long long)tail : launchSeq) % lanes); }
    int chunks_for(int frames) const { return (staged > 0 ? 1 : 0) + (frames + B - 1) / B; }

    Chunk next(int n) const
    {
        Chunk c;
        c.place = tail;
        c.lane = next_lane();
        c.area = next_area();
        c.pos0 = mini ? 1 : (ringPos + n <= ringFrames ? ringPos : 0);
        c.n = n;
        c.first = prevPos >= 0 ? 0 : 1;
        c.prevPos = prevPos;
        c.firstPair = pairCounter;
        c.epoch = epoch;
        return c;
    }

    // pairs submitted or staged and not popped yet (the caller adds what is left of the view it holds)
    int pending() const
    {
        int n = 0;
        for (const Place &p : place)
            if (p.state == 1) n += p.pairs;
        if (staged > 0) n += staged - (prevPos >= 0 ? 0 : 1);
        return n;
    }

    // ---- the transitions ----

    int stage_one() { return ++staged; }
    int take_staged()
    {
        const int n = staged;
        staged = 0; // (whatever happens to them, these frames are not submitted a second time)
        return n;
    }

    // the chunk is queued completely: it takes its place, its area, its slots and its pair numbers
    void commit(const Chunk &c)
    {
        Place &p = place[(size_t)c.place];
        p.state = 1, p.firstPair = c.firstPair, p.pairs = c.pairs(), p.epoch = c.epoch;
        tail = (tail + 1) % places();
        inFlight++;
        launchSeq++;
        chunkSeq++;
        pairCounter += c.pairs();
        keep_frames(c);
        loneLatest = false;
    }

    // a chunk of one frame without a predecessor: nothing to run, no place, no area -- it only becomes the latest frame
    void lone_first_frame(const Chunk &c)
    {
        keep_frames(c);
        loneLatest = true;
    }

    // the oldest chunk's results have been handed out: its place is free
    Place pop()
    {
        const Place p = place[(size_t)head];
        place[(size_t)head].state = 0;
        head = (head + 1) % places();
        inFlight--;
        return p;
    }

    // the next frame has no predecessor, pair numbering restarts at 0, the epoch advances (include/putslam_hip.h)
    void reset()
    {
        if (loneLatest && !mini) ringPos = prevPos; // (nothing has read that frame, and nothing will)
        loneLatest = false;
        prevPos = -1;
        pairCounter = 0;
        epoch++;
    }

    // a chunk could not be queued: its frames are dropped as a unit and the stream goes on as after reset(); places, rotation and
    // ring cursor are where the chunk found them
    void abort()
    {
        reset();
        staged = 0;
    }

private:
    void keep_frames(const Chunk &c)
    {
        ringPos = c.pos0 + c.n;
        prevPos = mini ? 0 : c.pos0 + c.n - 1;
    }
};

} // namespace psledger
