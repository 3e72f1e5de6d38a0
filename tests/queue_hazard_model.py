"""A model of the bookkeeping PsBatchQueue had BEFORE putslam_amd/csrc/ps_queue_hazard.h, kept as a fixture: one remembered output
block and batch number per chain (lastOut[chain], lastSeq[chain]), whole batches only.  A batch that a redirect brought to a chain
overwrote what the chain remembered, the batches on the forgotten block were still in flight there, and the next batch on that
block ran beside them on its nominal chain.  tests/test_queue_hazard_host.py runs every sequence of operations through this model
and through the safety check below -- the check of tests/cpp/test_queue_hazard.cpp, (a), for whole batches -- and finds the first
rejections exactly where the hole was: "A x chains, B, A".  A checker that cannot fail proves nothing; this one can.

Operations, as in the C++ program: a block's letter submits a whole batch on it, a digit completes the oldest unfinished batch of
that chain (first in, first out per chain, enforced here)."""


class OldQueue:
    def __init__(self, chains):
        self.chains = chains
        self.last_out = [None] * chains
        self.last_seq = [-1] * chains
        self.chain_of = []              # chain of every batch ever submitted
        self.block_of = []
        self.done = []

    def submit(self, block):
        """ps_batch_queue_submit's former chain choice for a whole batch.  Returns the chain."""
        seq = len(self.chain_of)
        mine = seq % self.chains
        for j in range(self.chains):
            if j == mine or self.last_out[j] != block or self.last_seq[j] < 0:
                continue
            if not self.done[self.last_seq[j]]:
                mine = j
                break
        self.last_out[mine], self.last_seq[mine] = block, seq
        self.chain_of.append(mine)
        self.block_of.append(block)
        self.done.append(False)
        return mine

    def complete(self, chain):
        """The oldest unfinished batch of the chain completes.  False if the chain has none."""
        for m, c in enumerate(self.chain_of):
            if c == chain and not self.done[m]:
                self.done[m] = True
                return True
        return False

    def unsafe(self):
        """The safety check for the batch submitted last, a direct scan: the earlier batches on its block that are not complete
        and sit on another chain.  Whole batches write all rows, and the old rule queued no cross-chain wait, so each of them runs
        beside the new batch."""
        n = len(self.chain_of) - 1
        return [m for m in range(n)
                if self.block_of[m] == self.block_of[n] and not self.done[m] and self.chain_of[m] != self.chain_of[n]]


def run(chains, ops):
    """ops: a string of block letters and chain digits.  Returns (index of the first operation the check rejects or None, the
    batches it ran beside, the chains of all batches)."""
    q = OldQueue(chains)
    for i, op in enumerate(ops):
        if op.isdigit():
            if not q.complete(int(op)):
                raise ValueError("chain %s has nothing to complete at operation %d of %r" % (op, i, ops))
        else:
            q.submit(op)
            bad = q.unsafe()
            if bad:
                return i, bad, q.chain_of
    return None, [], q.chain_of


def canonical(ops):
    """Blocks renamed in order of first use: "CCAC" -> "AABA"."""
    names = {}
    return "".join(op if op.isdigit() else names.setdefault(op, chr(ord("A") + len(names))) for op in ops)


def rejected_sequences(chains, max_length, blocks=3):
    """Every sequence of at most `max_length` operations over `blocks` blocks whose LAST operation is the first the check rejects,
    canonical: {length: sorted list}.  Sequences that ask a chain with nothing in flight to complete do not exist."""
    found = {n: set() for n in range(1, max_length + 1)}
    alphabet = [chr(ord("A") + b) for b in range(blocks)] + [str(c) for c in range(chains)]

    def go(prefix):
        if len(prefix) == max_length:
            return
        for op in alphabet:
            ops = prefix + op
            try:
                at, _, _ = run(chains, ops)
            except ValueError:
                continue
            if at is not None:
                found[len(ops)].add(canonical(ops))
                continue
            go(ops)

    go("")
    return {n: sorted(v) for n, v in found.items()}
