"""The restatement of cv::BFMatcher(cv::NORM_L2, crossCheck=true).match(query, train) (reference src/Matcher/matcherOpenCV.cpp:100-102,
198-206) that the float-descriptor matcher is held to, byte for byte.  THIS FILE IS THE DEFINITION; it is
unpinned against a real OpenCV, like the Hamming matcher's.

L2sqr(a, b) in float32, every operation rounded separately (numpy float32 arithmetic has no FMA), in the order of OpenCV 3.0 - 3.3's
SSE2 normL2Sqr_(const float*, const float*, int); dist = sqrtf(L2sqr) correctly rounded; every comparison on dist.
"""
import numpy as np

from putslam_amd import synth
from putslam_amd._abi import DMATCH_DTYPE

FLT_MAX = np.float32(3.4028234663852886e38)


def l2sqr_matrix(train, query):
    """(nt, D), (nq, D) float32 -> (nt, nq) float32 restated sums, all pairs at once (the order of operations per pair is the
    sequential one)."""
    train = np.ascontiguousarray(train, np.float32)
    query = np.ascontiguousarray(query, np.float32)
    nt, D = train.shape
    nq = query.shape[0]
    assert query.shape[1] == D and D >= 1

    def sq(j):
        t = train[:, j][:, None] - query[:, j][None, :]
        return t * t

    with np.errstate(all="ignore"):
        j = 0
        d = np.zeros((nt, nq), np.float32)
        if D >= 8:
            acc = [np.zeros((nt, nq), np.float32) for _ in range(8)]      # acc0[0..3], acc1[0..3]
            while j <= D - 8:
                for i in range(8):
                    acc[i] = acc[i] + sq(j + i)
                j += 8
            s = [acc[i] + acc[4 + i] for i in range(4)]
            d = ((s[0] + s[1]) + s[2]) + s[3]
        while j <= D - 4:
            d = d + (((sq(j) + sq(j + 1)) + sq(j + 2)) + sq(j + 3))
            j += 4
        while j < D:
            d = d + sq(j)
            j += 1
    assert d.dtype == np.float32
    return d


def l2sqr(a, b):
    """The restated sum of one pair of rows."""
    return l2sqr_matrix(np.asarray(a, np.float32)[None, :], np.asarray(b, np.float32)[None, :])[0, 0]


def dist_matrix(train, query):
    with np.errstate(all="ignore"):
        return np.sqrt(l2sqr_matrix(train, query))


def match_l2(query, train):
    """The cross-check match list (DMATCH_DTYPE, ascending queryIdx)."""
    query = np.asarray(query, np.float32)
    train = np.asarray(train, np.float32)
    nq, nt = query.shape[0], train.shape[0]
    if nq == 0 or nt == 0:
        return np.zeros(0, DMATCH_DTYPE)
    dist = dist_matrix(train, query)
    # step 1: strict '<' against FLT_MAX while q ascends = the first least admissible distance
    with np.errstate(all="ignore"):
        ok = dist < FLT_MAX
    masked = np.where(ok, dist, np.float32(np.inf))
    nn = np.where(ok.any(axis=1), masked.argmin(axis=1), -1)
    best = np.where(nn >= 0, masked[np.arange(nt), np.maximum(nn, 0)], FLT_MAX).astype(np.float32)
    # step 2
    qd = np.full(nq, FLT_MAX, np.float32)
    qi = np.full(nq, -1, np.int64)
    for t in range(nt):
        q = nn[t]
        if q >= 0 and best[t] < qd[q]:
            qd[q] = best[t]
            qi[q] = t
    # step 3
    keep = np.nonzero(qi >= 0)[0]
    out = np.zeros(keep.size, DMATCH_DTYPE)
    out["queryIdx"] = keep
    out["trainIdx"] = qi[keep]
    out["imgIdx"] = 0
    out["distance"] = qd[keep]
    return out


def match_l2_f64(query, train):
    """Float64 brute force of the same three steps (for well-separated data only: it rounds differently)."""
    q = np.asarray(query, np.float64)
    t = np.asarray(train, np.float64)
    d = np.sqrt(((t[:, None, :] - q[None, :, :]) ** 2).sum(axis=2))
    nn = d.argmin(axis=1)
    out = []
    for qq in range(q.shape[0]):
        ts = np.nonzero(nn == qq)[0]
        if ts.size:
            tt = ts[d[ts, qq].argmin()]
            out.append((qq, tt, d[tt, qq]))
    return out


def surf_scene(nq, nt, index=0):
    """SURF-like, D = 64: unit query rows; train = query + 0.08 N(0, 1) renormalised, 30 % fresh rows, permuted."""
    return synth.float_scene("surf", nq, nt, index)[:2]


def sift_scene(nq, nt, index=0):
    """SIFT-like, D = 128: query = |N(0, 1)| scaled to norm 512, floored, clipped to 0 .. 255; train = query + round(6 N(0, 1))
    clipped, 30 % fresh rows, permuted."""
    return synth.float_scene("sift", nq, nt, index)[:2]
