// ps_queue_hazard.h -- PsBatchQueue's bookkeeping (ps_batch_queue.cpp, include/putslam_hip.h), each rule once: which pairs of a batch
// go to which chain, and what a batch owes the batches still in flight that write the same output block.
// Pure -- no HIP header, no runtime call: tests/cpp/test_queue_hazard.cpp includes it into a plain C++ program and runs every
// sequence of submits and completions up to a fixed length through it.
//
// THE HAZARD.  Chains are HIP streams that nothing joins, so two batches on different chains run side by side; when they were handed
// the same output block (out->pose names it) they write the same rows of matches / numMatches / inlierMask / pose / stats, and the
// one the GPU happens to finish last wins.  What the queue promises instead is stream order: the block holds the results of the
// batch submitted last.  A SHARE is what one chain runs of a batch, pairs [bounds[c], bounds[c + 1]): a whole batch is one share, a
// split batch (PUTSLAM_HIP_QUEUE_SPLIT_FROM) one per chain.  An earlier share is IN FLIGHT while its event is not complete, and it
// concerns a new share when both write the block and their rows intersect.  A new share is ORDERED behind an earlier one when it runs
// on the same chain, or when its chain waits for the earlier share's event -- or for a later event of that chain: a chain completes
// its events in the order they were recorded.
//
// THE RULE (queue_hazard_plan), in this order:
//   1. no share in flight concerns a new share from ANOTHER chain: the nominal bounds, no wait.  A block with no writer in flight,
//      a batch that lands on its predecessors' chain by itself, and split batch after split batch with the same bounds end here.
//   2. the shares in flight that concern the batch all sit on ONE chain: the batch follows them on that chain, whole, no wait
//      -- as fast as one context, and no device-side wait is left pending (they cost the chains 5 - 19 %, profiles/r06v/pending_waits.txt).
//   3. they sit on several chains (whole after split, different splits): following cannot order them all.  A whole batch runs on
//      its nominal chain if that is one of them, else on the chain of the newest such share, and that chain waits for the newest
//      concerning event of each of the other chains; a split batch keeps its bounds and every share waits, per other chain, for the
//      newest event that concerns it.
// Every ticket still in the ring is looked at, not one per chain: a chain can hold batches on several blocks at once (a redirected
// batch brings a second block to the chain it follows to), and forgetting the older of them is how a later batch on that block
// came to run beside its predecessors.
#pragma once
#include <cstdint>

#include "putslam_hip.h"

constexpr int kQueueMaxChains = PS_BATCH_QUEUE_MAX_CHAINS;

// what a ticket keeps of its batch for the rule
struct QueueBatchRecord {
    const void *block = nullptr;              // the output block's key: out->pose
    int32_t bounds[kQueueMaxChains + 1] = {}; // pairs [bounds[c], bounds[c + 1]) on chain c
    bool used[kQueueMaxChains] = {};          // chain c ran a share and its event was recorded
};

// chain `waiter` must wait for the event of chain `chain` of the ticket `age` submits back (1 = the batch before this one)
struct QueueWait {
    int age, chain, waiter;
};

struct QueuePlan {
    int32_t bounds[kQueueMaxChains + 1] = {};
    int nwaits = 0;
    QueueWait waits[kQueueMaxChains * (kQueueMaxChains - 1)];
};

// THE NOMINAL BOUNDS of batch number `seq` of P pairs: whole on chain seq mod chains when P < splitFrom, else split -- two chains:
// splitPermille of the pairs on chain 0; more: equal shares.
inline void queue_nominal_bounds(int chains, int P, long long seq, int splitFrom, int splitPermille, int32_t *bounds)
{
    if (chains == 1) {
        bounds[0] = 0;
        bounds[1] = P;
        return;
    }
    if (P < splitFrom) {
        const int c = (int)(seq % chains);
        for (int i = 0; i <= chains; ++i) bounds[i] = i <= c ? 0 : P;
        return;
    }
    if (chains == 2) {
        bounds[0] = 0;
        bounds[1] = (int32_t)((long long)P * splitPermille / 1000);
        bounds[2] = P;
        return;
    }
    for (int i = 0; i <= chains; ++i) bounds[i] = (int32_t)((long long)P * i / chains);
}

inline void queue_whole_on(int chains, int chain, int P, int32_t *bounds)
{
    for (int i = 0; i <= chains; ++i) bounds[i] = i <= chain ? 0 : P;
}

// THE RULE above.  `nominal`: queue_nominal_bounds of the batch; `block`: its key; `tickets`: how many earlier batches the ring still
// holds; record(age) -> const QueueBatchRecord * of the batch `age` submits back (1 .. tickets), or nullptr for a slot without one;
// complete(age, chain) -> whether that batch's event on that chain has happened (asked only where used[chain], newest first, never
// below a complete event of the same chain -- what a chain recorded before it is complete as well -- and never where the answer
// could not change the plan: older shares of a chain whose newer share in flight already concerns the same shares of the batch).
template <class Record, class Complete>
inline void queue_hazard_plan(int chains, const int32_t *nominal, const void *block, int tickets, Record record, Complete complete,
                              QueuePlan &plan)
{
    plan.nwaits = 0;
    for (int i = 0; i <= chains; ++i) plan.bounds[i] = nominal[i];
    const int32_t P = nominal[chains];
    if (chains < 2 || P <= 0) return;

    // newest[w][c]: the newest share in flight on chain c whose rows intersect rows w -- w < chains: the nominal share of chain w;
    // w == chains: the whole batch, [0, P) -- as an age, 0 for none
    int newest[kQueueMaxChains + 1][kQueueMaxChains] = {};
    bool drained[kQueueMaxChains] = {};
    for (int age = 1; age <= tickets; ++age) {
        const QueueBatchRecord *r = record(age);
        if (!r || r->block != block) continue;
        for (int c = 0; c < chains; ++c) {
            const int32_t lo = r->bounds[c], hi = r->bounds[c + 1];
            if (!r->used[c] || drained[c] || hi <= lo || lo >= P) continue;
            bool news = !newest[chains][c]; // (a host that keeps a block on its chain has one event asked per submit, not one per ticket)
            for (int w = 0; w < chains; ++w) news = news || (!newest[w][c] && nominal[w] < nominal[w + 1] && lo < nominal[w + 1] && nominal[w] < hi);
            if (!news) continue;
            if (complete(age, c)) {
                drained[c] = true;
                continue;
            }
            if (!newest[chains][c]) newest[chains][c] = age;
            for (int w = 0; w < chains; ++w)
                if (!newest[w][c] && nominal[w] < nominal[w + 1] && lo < nominal[w + 1] && nominal[w] < hi) newest[w][c] = age;
        }
    }

    int nominalChain = -1, shares = 0;
    bool hazard = false;
    for (int w = 0; w < chains; ++w) {
        if (nominal[w + 1] <= nominal[w]) continue;
        ++shares;
        nominalChain = w;
        for (int c = 0; c < chains; ++c) hazard = hazard || (c != w && newest[w][c]);
    }
    if (!hazard) return; // 1.

    int writers = 0, last = -1, youngest = -1;
    for (int c = 0; c < chains; ++c)
        if (newest[chains][c]) {
            ++writers;
            last = c;
            if (youngest < 0 || newest[chains][c] < newest[chains][youngest]) youngest = c;
        }
    if (writers == 1) { // 2.
        queue_whole_on(chains, last, P, plan.bounds);
        return;
    }
    if (shares == 1) { // 3., whole
        const int mine = newest[chains][nominalChain] ? nominalChain : youngest;
        queue_whole_on(chains, mine, P, plan.bounds);
        for (int c = 0; c < chains; ++c)
            if (c != mine && newest[chains][c]) plan.waits[plan.nwaits++] = QueueWait{newest[chains][c], c, mine};
        return;
    }
    for (int w = 0; w < chains; ++w) { // 3., split
        if (nominal[w + 1] <= nominal[w]) continue;
        for (int c = 0; c < chains; ++c)
            if (c != w && newest[w][c]) plan.waits[plan.nwaits++] = QueueWait{newest[w][c], c, w};
    }
}
