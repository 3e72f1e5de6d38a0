// The pipelined stream's ledger and result layout (putslam_amd/csrc/ps_stream_ledger.h) on the host, no HIP, no GPU.
//
//   (no argument)  random call sequences -- chunks of 1..B frames, lone first frames, frames staged one at a time up to a flush,
//                  pops, resets, chunks that fail before their commit -- over both forms, lanes 2..8, ahead 0..4 and B in
//                  {1, 2, 4, 5, 47, 48, 128}, beside a model of the chunks ALIVE (committed, not popped): what is handed to a new
//                  chunk -- staging area / upload event, ring slots, place -- is nothing a chunk alive reads; places go round in
//                  order; room() counts the free ones; pair numbers and epochs follow include/putslam_hip.h.  On the sequences
//                  without a failing chunk every value also equals the expressions ps_stream_async.h held before the ledger
//                  (restated in ParentModel below), step by step.
//   layout         ResLayout against async_build's expressions and the three hand-written forms of a partly filled chunk's
//                  five segments.
//
// Two deliberate differences from those expressions, both forced by the slot assertion and both about resets.  The ring has
// one more slot per place ((lanes + ahead + 2) x B + lanes + ahead: every chunk alive may follow a lone first frame, which
// took a slot and no place), so the wrap rule is restated over the ledger's ringFrames.  And a lone first frame that a reset
// drops hands its slot back: before, every reset + frame without a chunk between moved the cursor one slot on while no place
// was taken, and a few of them walked it into slots chunks alive still read.  From the first such drop of a sequence on, the
// ring positions are compared through the wrap rule applied to the ledger's own cursor.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <random>
#include <vector>

#include "ps_stream_ledger.h"

using psledger::Chunk;
using psledger::Ledger;
using psledger::Place;
using psledger::ResLayout;

#define CHECK(cond)                                                                                       \
    do {                                                                                                  \
        if (!(cond)) {                                                                                    \
            fprintf(stderr, "%s:%d: %s   [sequence %ld, step %d: %s]\n", __FILE__, __LINE__, #cond, g_seq, g_step, g_cfg); \
            exit(1);                                                                                      \
        }                                                                                                 \
    } while (0)

static long g_seq = 0;
static int g_step = 0;
static char g_cfg[96] = "";

// ---- what ps_stream_async.h computed before the ledger, restated (sequences without a failing chunk) ----
struct ParentModel {
    int B, lanes, ahead, ringFrames, S;
    bool mini;
    std::vector<int> state, pairs;
    int head = 0, tail = 0;
    long long launchSeq = 0, chunkSeq = 0, pairCounter = 0;
    int ringPos = 0, prevPos = -1, epoch = 0, staged = 0;
    ParentModel(int B_, int lanes_, int ahead_, bool mini_, int ringFrames_) : B(B_), lanes(lanes_), ahead(ahead_), ringFrames(ringFrames_), mini(mini_)
    {
        S = lanes + ahead;
        state.assign((size_t)S, 0);
        pairs.assign((size_t)S, 0);
    }
    int room() const
    {
        int freePlaces = 0;
        for (int i = 0; i < S && state[(size_t)((tail + i) % S)] == 0; ++i) ++freePlaces;
        return freePlaces;
    }
    int stage_area() const { return (int)(chunkSeq % (long long)(lanes + ahead + 1)); }
    int pending() const
    {
        int n = 0;
        for (int i = 0; i < S; ++i)
            if (state[(size_t)i] == 1) n += pairs[(size_t)i];
        if (staged > 0) n += staged - (prevPos >= 0 ? 0 : 1);
        return n;
    }
    struct Out {
        int pos0, first, prevPos, area, lane, place, epoch;
        long long firstPair;
        std::vector<int> pairList;
    };
    // async_submit_body + async_launch / mini_submit_body; ringCursor >= 0: the ring position to apply the wrap rule to
    Out submit(int n, int ringCursor)
    {
        Out o;
        o.place = tail;
        o.epoch = epoch;
        o.firstPair = pairCounter;
        if (!mini) {
            if (ringCursor >= 0) ringPos = ringCursor;
            const int pos0 = (ringPos + n <= ringFrames) ? ringPos : 0;
            o.area = (int)(chunkSeq % (long long)(lanes + ahead + 1));
            chunkSeq++;
            o.pos0 = pos0;
            o.first = prevPos >= 0 ? 0 : 1;
            o.prevPos = prevPos;
            for (int i = o.first; i < n; ++i) {
                o.pairList.push_back(i == 0 ? o.prevPos : pos0 + i - 1);
                o.pairList.push_back(pos0 + i);
            }
            const int P = n - o.first;
            ringPos = pos0 + n;
            prevPos = pos0 + n - 1;
            o.lane = (int)(launchSeq % (long long)lanes);
            if (P <= 0) {
                chunkSeq--;
                return o;
            }
            pairCounter += P;
            commit(P);
        } else {
            o.area = (int)(chunkSeq % (long long)(lanes + ahead + 1));
            o.first = prevPos >= 0 ? 0 : 1;
            o.prevPos = prevPos;
            o.pos0 = 1;
            const int P = n - o.first;
            o.lane = tail % lanes;
            if (P <= 0) {
                prevPos = 0;
                return o;
            }
            chunkSeq++;
            prevPos = 0;
            for (int i = 0; i < P; ++i) {
                o.pairList.push_back(o.first + i);
                o.pairList.push_back(o.first + i + 1);
            }
            commit(P);
            pairCounter += P;
        }
        return o;
    }
    void commit(int P)
    {
        state[(size_t)tail] = 1;
        pairs[(size_t)tail] = P;
        launchSeq++;
        tail = (tail + 1) % S;
    }
    void pop()
    {
        state[(size_t)head] = 0;
        head = (head + 1) % S;
    }
    void reset()
    {
        prevPos = -1;
        pairCounter = 0;
        epoch++;
    }
};

// ---- the chunks alive, and what each reads ----
struct Live {
    int place, area, haloArea; // haloArea: a mini chunk reads its predecessor's last frame there (-1: none / not in an area)
    int pos0, n, haloSlot;     // ring form: its slots and its predecessor's (-1: none)
    long long firstPair;
    int pairs, epoch;
};

struct Harness {
    Ledger L;
    ParentModel par;
    std::deque<Live> live;
    bool compare;         // no failing chunk in this sequence: every value equals the parent's
    bool dropped = false; // a reset has dropped a lone first frame: ring positions through the wrap rule from here on
    long long commits = 0, pops = 0;
    // the contract of include/putslam_hip.h, counted independently
    long long wantPair = 0;
    int wantEpoch = 0;
    bool haveFrame = false;
    int latestArea = -1, latestSlot = -1;

    Harness(int B, int lanes, int ahead, bool mini, bool compare_) : par(B, lanes, ahead, mini, 0), compare(compare_)
    {
        L.configure(B, lanes, ahead, mini);
        par.ringFrames = L.ringFrames;
        CHECK(L.places() == lanes + ahead && L.areas() == lanes + ahead + 1 && (mini || L.ringFrames >= (lanes + ahead + 2) * B));
    }

    void check_counts()
    {
        CHECK(L.room() == L.places() - (int)live.size());
        CHECK(L.inFlight == (int)live.size());
        int freeFromTail = 0;
        for (int i = 0; i < L.places() && L.place[(size_t)((L.tail + i) % L.places())].state == 0; ++i) ++freeFromTail;
        CHECK(freeFromTail == L.room()); // (the free places are the ones from tail on)
        if (compare) {
            CHECK(L.room() == par.room());
            CHECK(L.pending() == par.pending());
            CHECK(L.next_area() == par.stage_area());
            CHECK(L.staged == par.staged);
        }
    }

    // n frames become a chunk (or a lone first frame); `fails`: the chunk cannot be queued
    void submit(int n, bool fails)
    {
        const Chunk c = L.next(n);
        CHECK(c.n == n && c.first == (haveFrame ? 0 : 1) && c.epoch == wantEpoch && c.firstPair == wantPair);
        CHECK(c.area == L.next_area() && c.area >= 0 && c.area < L.areas());
        if (!L.mini) {
            CHECK(c.pos0 >= 0 && c.pos0 + n <= L.ringFrames);
            CHECK(c.first || c.prevPos == latestSlot);
            for (const Live &v : live) { // the slots written are not read by a chunk alive, as its own or as its previous frame
                CHECK(c.pos0 + n <= v.pos0 || v.pos0 + v.n <= c.pos0);
                CHECK(v.haloSlot < c.pos0 || v.haloSlot >= c.pos0 + n);
            }
            CHECK(c.first || c.prevPos < c.pos0 || c.prevPos >= c.pos0 + n);
        } else {
            CHECK(c.pos0 == 1 && (c.first || c.prevPos == 0));
        }
        ParentModel::Out o;
        if (compare) {
            o = par.submit(n, dropped ? L.ringPos : -1);
            CHECK(c.pos0 == o.pos0 && c.first == o.first && c.prevPos == o.prevPos && c.firstPair == o.firstPair && c.epoch == o.epoch);
            CHECK((int)o.pairList.size() == 2 * c.pairs() || c.pairs() <= 0);
            for (int i = c.first; i < n; ++i) CHECK(c.query(i) == o.pairList[(size_t)(2 * (i - c.first))] && c.train(i) == o.pairList[(size_t)(2 * (i - c.first) + 1)]);
        }
        if (c.pairs() <= 0) {
            L.lone_first_frame(c);
            haveFrame = true;
            latestArea = -1; // (ring: in the ring; mini: in a block of its own, guarded by an event)
            latestSlot = L.mini ? -1 : c.pos0;
            CHECK(L.prevPos >= 0);
            return;
        }
        // a place, an area and an upload event are taken: none that a chunk alive holds or reads
        CHECK(L.room() >= 1 && c.place == L.tail && L.place[(size_t)c.place].state == 0);
        CHECK(c.place == (int)(commits % L.places()));
        CHECK(c.lane >= 0 && c.lane < L.lanes && c.lane == (L.mini ? c.place % L.lanes : (int)(commits % L.lanes)));
        for (const Live &v : live) CHECK(c.area != v.area && c.area != v.haloArea && c.place != v.place);
        if (compare) CHECK(c.area == o.area && c.lane == o.lane && c.place == o.place);
        if (fails) {
            const Ledger before = L;
            L.abort();
            // places, rotation and ring cursor are where the chunk found them; the stream goes on as after a reset
            CHECK(L.chunkSeq == before.chunkSeq && L.launchSeq == before.launchSeq && L.tail == before.tail && L.head == before.head &&
                  L.inFlight == before.inFlight && L.staged == 0 && L.prevPos == -1 && L.pairCounter == 0 && L.epoch == before.epoch + 1);
            CHECK(L.ringPos == before.ringPos || (before.loneLatest && L.ringPos == before.prevPos));
            wantEpoch++, wantPair = 0, haveFrame = false, latestArea = latestSlot = -1;
            return;
        }
        L.commit(c);
        commits++;
        Live v;
        v.place = c.place, v.area = c.area, v.haloArea = (L.mini && !c.first) ? latestArea : -1;
        v.pos0 = L.mini ? 0 : c.pos0, v.n = L.mini ? 0 : n, v.haloSlot = (!L.mini && !c.first) ? c.prevPos : -1;
        v.firstPair = c.firstPair, v.pairs = c.pairs(), v.epoch = c.epoch;
        live.push_back(v);
        wantPair += c.pairs();
        haveFrame = true;
        latestArea = c.area;
        latestSlot = L.mini ? -1 : c.pos0 + n - 1;
    }

    void submit_staged(bool fails)
    {
        if (L.staged == 0) return;
        const int n = L.take_staged();
        if (compare) par.staged = 0;
        submit(n, fails);
    }

    bool push_chunk(int n, bool fails) // push_many's rule: all or nothing
    {
        if (L.chunks_for(n) > L.room()) return false;
        submit_staged(false);
        submit(n, fails);
        return true;
    }

    bool stage_one() // push_async
    {
        if (L.staged == 0 && L.room() < 1) return false;
        if (compare) par.staged++;
        if (L.stage_one() == L.B) submit_staged(false);
        return true;
    }

    bool pop()
    {
        if (L.inFlight == 0) return false;
        CHECK(!live.empty());
        const Live v = live.front();
        live.pop_front();
        CHECK(L.head == v.place && v.place == (int)(pops % L.places())); // oldest first, places in order
        const Place p = L.pop();
        pops++;
        CHECK(p.state == 1 && p.firstPair == v.firstPair && p.pairs == v.pairs && p.epoch == v.epoch);
        if (compare) par.pop();
        return true;
    }

    void reset()
    {
        submit_staged(false);
        if (L.loneLatest && !L.mini) dropped = true;
        L.reset();
        if (compare) par.reset();
        wantEpoch++, wantPair = 0, haveFrame = false, latestArea = latestSlot = -1;
    }
};

static int run_sequences(long sequences)
{
    static const int Bs[7] = {1, 2, 4, 5, 47, 48, 128};
    long chunks = 0, lone = 0, failed = 0, drops = 0, busy = 0;
    for (g_seq = 0; g_seq < sequences; ++g_seq) {
        std::mt19937_64 rng(0x57A3A11ull + (unsigned long long)g_seq);
        auto pick = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned long long)(hi - lo + 1)); };
        const int B = Bs[g_seq % 7], lanes = pick(2, 8), ahead = pick(0, 4);
        const bool mini = (g_seq / 7) % 2 == 0, withFailures = (g_seq / 14) % 2 == 0;
        // (the library takes the mini form for chunks of up to four frames; the ledger's rules do not depend on B, so both forms run every B)
        snprintf(g_cfg, sizeof g_cfg, "B %d lanes %d ahead %d %s%s", B, lanes, ahead, mini ? "mini" : "ring", withFailures ? " with failures" : "");
        Harness h(B, lanes, ahead, mini, !withFailures);
        const int steps = pick(40, 160);
        // (small chunks and frequent resets are where the rotation went wrong before: every other sequence leans that way)
        const bool small = g_seq % 3 == 0;
        for (g_step = 0; g_step < steps; ++g_step) {
            h.check_counts();
            const int op = pick(0, 99);
            const int n = small ? pick(1, B < 2 ? 1 : 2) : pick(1, B);
            if (op < 30) {
                if (h.push_chunk(n, false)) chunks++;
                else busy++;
            } else if (op < 50) {
                if (!h.stage_one()) busy++;
            } else if (op < 55) {
                h.submit_staged(false); // flush
            } else if (op < 78) {
                h.pop();
            } else if (op < 86) {
                h.reset();
            } else if (op < 93) { // a lone first frame: reset, then one frame
                h.reset();
                if (h.push_chunk(1, false)) lone++;
            } else if (withFailures) {
                if (h.push_chunk(n, true)) failed++;
            }
        }
        while (h.pop()) {}
        h.check_counts();
        CHECK(h.L.pending() == (h.L.staged > 0 ? h.L.staged - (h.L.prevPos >= 0 ? 0 : 1) : 0));
        drops += h.dropped ? 1 : 0;
    }
    printf("stream ledger ok: %ld sequences, %ld chunks, %ld lone frames, %ld failed chunks, %ld refused for room, %ld sequences with a dropped lone frame\n",
           sequences, chunks, lone, failed, busy, drops);
    return 0;
}

static int run_layout()
{
    g_seq = -1;
    static const size_t Bs[5] = {1, 4, 5, 128, 1024}, caps[4] = {1, 600, 2000, PS_MAX_KPTS};
    for (size_t B : Bs)
        for (size_t cap : caps) {
            snprintf(g_cfg, sizeof g_cfg, "B %zu cap %zu", B, cap);
            const ResLayout r(B, cap);
            // async_build's expressions
            const size_t offMask = B * cap * sizeof(PsDMatch);
            const size_t offPose = offMask + ((B * cap + 63) & ~(size_t)63);
            const size_t offStats = offPose + B * 64;
            const size_t offNum = offStats + ((B * sizeof(PsRansacStats) + 63) & ~(size_t)63);
            const size_t resBytes = offNum + B * sizeof(int32_t);
            CHECK(r.cap == cap && r.offMask == offMask && r.offPose == offPose && r.offStats == offStats && r.offNum == offNum && r.bytes == resBytes);
            CHECK(r.alloc_bytes() == ((resBytes + 15) & ~(size_t)15));
            // the views
            std::vector<uint8_t> dummy(1);
            uint8_t *base = dummy.data();
            const PsPairResults d = r.device(base);
            CHECK((uint8_t *)d.matches == base && d.inlierMask == base + offMask && (uint8_t *)d.pose == base + offPose &&
                  (uint8_t *)d.stats == base + offStats && (uint8_t *)d.numMatches == base + offNum);
            for (int mode = PS_RESULTS_FULL; mode <= PS_RESULTS_POSES; ++mode) {
                PsHostPairResults h;
                memset(&h, 0, sizeof h);
                r.host(base, mode, &h);
                CHECK(h.matches == (mode == PS_RESULTS_POSES ? nullptr : (const PsDMatch *)base));
                CHECK(h.inlierMask == (mode == PS_RESULTS_FULL ? base + offMask : nullptr));
                CHECK(h.resultMode == mode && (const uint8_t *)h.pose == base + offPose && (const uint8_t *)h.stats == base + offStats &&
                      (const uint8_t *)h.numMatches == base + offNum);
            }
            const size_t Ps[3] = {1, B > 1 ? B - 1 : 1, B};
            for (size_t p : Ps) {
                const size_t off[5] = {0, offMask, offPose, offStats, offNum};
                // the hipMemcpyAsync calls of a partly filled chunk and pop_many's memcpy calls ...
                const size_t plain[5] = {p * cap * sizeof(PsDMatch), p * cap, p * 64, p * sizeof(PsRansacStats), p * sizeof(int32_t)};
                // ... and the CopySegs table of a mini chunk's results
                const size_t len[5] = {p * cap * sizeof(PsDMatch), (p * cap + 3) & ~(size_t)3, p * 64, p * sizeof(PsRansacStats), p * sizeof(int32_t)};
                ResLayout::Seg s1[5], s4[5];
                r.segments(p, 1, s1);
                r.segments(p, 4, s4);
                for (int k = 0; k < 5; ++k) {
                    CHECK(s1[k].off == off[k] && s1[k].bytes == plain[k]);
                    CHECK(s4[k].off == off[k] && s4[k].bytes == len[k]);
                    CHECK(s4[k].off + s4[k].bytes <= (k < 4 ? off[k + 1] : r.alloc_bytes())); // (a rounded segment stays inside its own)
                }
            }
        }
    printf("result layout ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "layout")) return run_layout();
    return run_sequences(argc > 1 ? atol(argv[1]) : 24000);
}
