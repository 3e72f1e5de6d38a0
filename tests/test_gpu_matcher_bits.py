"""Kernel 1 at the smallest shapes at which its chunked, load-ahead form can go wrong, in all three forms: the FP4 matrix-core
sweep that expands the query tiles itself (ps_hamming_mfma_fused), the same sweep reading an FP4 image (ps_hamming_mfma) and
the integer VALU sweep (ps_hamming_nn).  Every list is held against the cross-check restated here from XOR + popcount (no
reference program involved), so the three forms' keys (hamming << 16 | query, ties to the lowest query) agree with it and
with one another.

The fused kernel cuts a sweep of nq query rows into chunks of four whole 32-row tiles, loads the descriptor dwords of a chunk
two chunks ahead, and handles what is left -- up to three whole tiles and the partial tile -- outside its main loop.  The frame
sizes below cover: no whole tile (1, 31), one whole tile and nothing else (32), a partial tile behind a whole one (33), a tail
of three whole tiles and a partial one (127), exactly one chunk (128), a partial tile straight after a whole chunk (129), a chunk
plus one whole tile (160), two chunks plus a partial tile (257: the load-ahead of two chunks ends here) and two chunks, a whole
tile and a partial one (289)."""
import numpy as np
import pytest

from putslam_amd import api
from putslam_amd._abi import DMATCH_DTYPE, EST_RANSAC, TUM_FR1_K, default_ransac_params, make_config
from putslam_amd.device_batch import FrameSetDevice, PackedFrameSetDevice, PairBatchDevice, run_pairs

pytestmark = pytest.mark.gpu

FORMS = [("mfma-fused", 1, 1), ("mfma-image", 1, 0), ("valu", 0, 0)]
SIZES = [1, 31, 32, 33, 127, 128, 129, 160, 257, 289]


@pytest.fixture(scope="module", params=FORMS, ids=[f[0] for f in FORMS])
def fctx(request):
    c = api.Context(0)
    c.set_option("matcher", request.param[1])
    c.set_option("matcher_fused", request.param[2])
    yield c
    c.close()


def _bits(rows):
    return np.unpackbits(np.ascontiguousarray(rows, np.uint8), axis=1).astype(np.float32)


def restated(q, t):
    """BFMatcher(NORM_HAMMING, crossCheck=true) from XOR + popcount: for every train row the nearest query row, ties to the
    lowest query; of the train rows that chose a query the nearest stays, ties to the lowest train; listed by query."""
    out = np.zeros(0, DMATCH_DTYPE)
    if len(q) == 0 or len(t) == 0:
        return out
    a, b = _bits(q), _bits(t)
    d = np.rint(a @ (1.0 - b).T + (1.0 - a) @ b.T).astype(np.int64)      # (nq, nt) popcount(q ^ t), exact in f32 (<= 256)
    bq = d.argmin(axis=0)                                                 # (first minimum = lowest query)
    best = d[bq, np.arange(len(t))]
    rows = []
    for qi in np.unique(bq):
        ts = np.nonzero(bq == qi)[0]
        ti = ts[best[ts].argmin()]
        rows.append((qi, ti, 0, float(best[ti])))
    return np.array(rows, DMATCH_DTYPE)


_PRM = default_ransac_params(0)
_CFG, _KEEP = make_config(EST_RANSAC, 487, seed=3)


def run_batch(c, desc, nkpts, pairs, stride=None):
    """The match lists of one batched call (the RANSAC behind them is not looked at)."""
    desc = np.array(desc, np.uint8)                              # (a copy: the shared frames stay read-only)
    F, cap = desc.shape[:2]
    pts = np.random.default_rng(1).uniform(0.5, 3.0, (F, cap, 3)).astype(np.float32)
    fs = FrameSetDevice(desc, pts, nkpts) if stride is None else PackedFrameSetDevice(desc, pts, nkpts, stride=stride)
    pb = PairBatchDevice(np.asarray(pairs, np.int32).reshape(-1, 2), cap)
    run_pairs(c, _PRM, _CFG, TUM_FR1_K, fs, pb, use_torch_stream=False)
    c.synchronize()
    got = pb.download()
    return [got["matches"][p][:int(got["numMatches"][p])] for p in range(len(pairs))]


_CACHE = {}


def sized_frames():
    """One frame per size of SIZES (capacity 289), every ordered pair of them; rows drawn from 48 base rows with a few bits
    flipped, so that equal and nearly equal distances are the rule.  Built once, with its restated lists."""
    if "sized" not in _CACHE:
        rng = np.random.default_rng(20261)
        cap = max(SIZES)
        base = rng.integers(0, 256, (48, 32), dtype=np.uint8)
        desc = base[rng.integers(0, 48, (len(SIZES), cap))] ^ np.packbits(rng.random((len(SIZES), cap, 256)) < 0.01, axis=2)
        pairs = [(a, b) for a in range(len(SIZES)) for b in range(len(SIZES))]
        want = [restated(desc[a][:SIZES[a]], desc[b][:SIZES[b]]) for a, b in pairs]
        desc.setflags(write=False)
        _CACHE["sized"] = (desc, np.array(SIZES, np.int32), pairs, want)
    return _CACHE["sized"]


def check_lists(got, want, pairs, what):
    for p, (g, w) in enumerate(zip(got, want)):
        assert g.tobytes() == w.tobytes(), (what, pairs[p], g[:4], w[:4])


@pytest.mark.parametrize("qsplit", [0, 1, 2, 3, 5])
def test_frame_sizes(fctx, qsplit):
    """nq, nt over SIZES, nq != nt included, in one call per query split: 0 = the library's own choice, 1 = one work-group
    sweeps every tile, 2 / 3 / 5 = sweeps that start in the middle of a frame, end before its last tile or are empty
    (merged with atomicMin)."""
    desc, nk, pairs, want = sized_frames()
    fctx.set_option("debug.qsplit", qsplit)
    try:
        got = run_batch(fctx, desc, nk, pairs)
    finally:
        fctx.set_option("debug.qsplit", 0)
    check_lists(got, want, pairs, "qsplit %d" % qsplit)


def test_pitched_frame_set(fctx):
    """The same frames with every frame's descriptors and points in one block and a frame stride greater than the rows need."""
    desc, nk, pairs, want = sized_frames()
    cap = desc.shape[1]
    stride = ((cap * 44 + 15) // 16) * 16 + 4096 + 48
    assert stride // 4 > cap * 8
    check_lists(run_batch(fctx, desc, nk, pairs, stride=stride), want, pairs, "pitched")


def test_every_descriptor_bit(fctx):
    """For each of the 256 bit positions b: the query frame holds the all-zero row and the row with only bit b set, the train
    frame the same two rows in the other order -- both nearest distances are 0 and the indices cross; and the row with only
    bit b set against the all-zero row alone, either way round -- the distance is exactly 1.  A wrong or one-sided assignment
    of descriptor bits to FP4 elements shows as a distance of 2 or a swapped index.  768 pairs of one call."""
    e = np.zeros((256, 256), np.uint8)
    e[np.arange(256), np.arange(256)] = 1
    e = np.packbits(e, axis=1)                                   # (256, 32): row b has bit b only
    desc = np.zeros((3 * 256 + 1, 8, 32), np.uint8)               # (capacity 8: rows 2.. are never read)
    desc[0:256, 1] = e                                           # frames 0..255: [zero, e_b]
    desc[256:512, 0] = e                                         # frames 256..511: [e_b, zero]
    desc[512:768, 0] = e                                         # frames 512..767: [e_b] alone
    nk = np.array([2] * 512 + [1] * 257, np.int32)               # frame 768: [zero] alone
    pairs = [(b, 256 + b) for b in range(256)] + [(512 + b, 768) for b in range(256)] + [(768, 512 + b) for b in range(256)]
    got = run_batch(fctx, desc, nk, pairs)
    crossed = np.array([(0, 1, 0, 0.0), (1, 0, 0, 0.0)], DMATCH_DTYPE)
    one = np.array([(0, 0, 0, 1.0)], DMATCH_DTYPE)
    for p, g in enumerate(got):
        w = crossed if p < 256 else one
        assert g.tobytes() == w.tobytes(), (pairs[p], p % 256, g)
        f0, f1 = pairs[p]
        assert w.tobytes() == restated(desc[f0][:nk[f0]], desc[f1][:nk[f1]]).tobytes()


def test_ties_within_and_across_tiles(fctx):
    """Duplicate query rows at positions 0, 31, 32 and 63 of a 64-row frame: the lowest index wins inside a tile (0 over 31,
    32 over 63) and across tiles (0 or 31 over 32 and 63), at distance 0 and at distance 1."""
    rng = np.random.default_rng(64)
    x = rng.integers(0, 256, 32, dtype=np.uint8)
    frames, lowest = [], []
    for dup in ((0, 31, 32, 63), (31, 32, 63), (32, 63), (63, ), (31, 63), (0, 63)):
        q = rng.integers(0, 256, (64, 32), dtype=np.uint8)
        q[list(dup)] = x
        frames.append(q)
        lowest.append(dup[0])
    t = rng.integers(0, 256, (64, 32), dtype=np.uint8)
    t[0] = x                                                     # distance 0 to every duplicate
    t[1] = x
    t[1, 7] ^= 0x10                                              # distance 1 to every duplicate
    t[40] = x
    t[40, 31] ^= 0x81                                            # distance 2
    frames.append(t)
    desc = np.stack(frames)
    nk = np.full(len(frames), 64, np.int32)
    pairs = [(i, len(frames) - 1) for i in range(len(lowest))]
    got = run_batch(fctx, desc, nk, pairs)
    for p, g in enumerate(got):
        assert g.tobytes() == restated(desc[p], t).tobytes(), (p, g[:4])
        hit = g[g["trainIdx"] == 0]
        assert len(hit) == 1 and hit[0]["queryIdx"] == lowest[p] and hit[0]["distance"] == 0.0, (p, g[:4])
        assert not np.any(np.isin(g["trainIdx"], (1, 40)))       # (they chose the same query at a greater distance)


def test_both_ends_of_the_key_range(fctx):
    """An all-equal pair of frames (every distance 0) and a complementary pair (every distance 256): one match each, query 0
    with train 0, at sizes with a partial tile behind whole chunks and with whole tiles only."""
    x = np.random.default_rng(9).integers(0, 256, 32, dtype=np.uint8)
    desc = np.stack([np.tile(x, (160, 1)), np.tile(x, (160, 1)), np.tile(~x, (160, 1))])
    nk = np.array([129, 160, 160], np.int32)
    pairs = [(0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (1, 1)]
    got = run_batch(fctx, desc, nk, pairs)
    for p, (g, (a, b)) in enumerate(zip(got, pairs)):
        d = 256.0 if 2 in (a, b) and a != b else 0.0
        assert g.tobytes() == np.array([(0, 0, 0, d)], DMATCH_DTYPE).tobytes(), (pairs[p], g)
        assert g.tobytes() == restated(desc[a][:nk[a]], desc[b][:nk[b]]).tobytes()
