"""DBScan::run (reference src/Matcher/dbscan.cpp) restated in numpy: the yardstick of the GPU kernel (ps_dbscan.h) and, through
tests/golden/dbscan_reference.npz, itself pinned to the reference's own code.

The restatement follows the reading of DESIGN.md section 8.1: the neighbour predicate exactly as the reference evaluates it
(float differences, cv::norm in double, the root rounded to float, compared with the double eps), the main loop in ascending
index, expansion through a deduplicated FIFO (a duplicate in the reference's list is a no-op), noise never relabelled, and the
keep rule with the -5 octave marker."""
from collections import deque

import numpy as np


def neighbour_matrix(xy, eps, block=512):
    """adj[i, k] = (double)(float)sqrt((double)dx*dx + (double)dy*dy) < eps with dx = x_i - x_k in float."""
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    n = xy.shape[0]
    adj = np.zeros((n, n), bool)
    with np.errstate(all="ignore"):
        for a in range(0, n, block):
            dx = (xy[a:a + block, 0][:, None] - xy[None, :, 0]).astype(np.float64)
            dy = (xy[a:a + block, 1][:, None] - xy[None, :, 1]).astype(np.float64)
            d = np.sqrt(dx * dx + dy * dy).astype(np.float32).astype(np.float64)
            adj[a:a + block] = d < eps
    return adj


def dbscan_labels(adj, min_pts):
    """Cluster labels as the reference leaves them: -1 noise, 1, 2, ... in the order the clusters were opened."""
    n = adj.shape[0]
    visited = np.zeros(n, bool)
    queued = np.zeros(n, bool)
    label = np.zeros(n, np.int64)
    c = 1
    for i in range(n):
        if visited[i]:
            continue
        visited[i] = True
        nb = np.flatnonzero(adj[i])
        if len(nb) < min_pts:
            label[i] = -1
            continue
        label[i] = c
        q = deque()
        new = nb[~visited[nb] & ~queued[nb]]
        queued[new] = True
        q.extend(new.tolist())
        while q:
            x = q.popleft()
            visited[x] = True
            cand = np.flatnonzero(adj[x] & ~visited)
            if len(cand) >= min_pts:
                new = cand[~queued[cand]]
                queued[new] = True
                q.extend(new.tolist())
            if label[x] == 0:
                label[x] = c
        c += 1
    return label


def dbscan_keep(xy, octave=None, eps=10.0, min_pts=2, features_from_cluster=1):
    """Indices (ascending, int32) of the keypoints DBScan(eps, min_pts, features_from_cluster).run leaves in the vector."""
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    n = xy.shape[0]
    if n == 0:
        return np.zeros(0, np.int32)
    label = dbscan_labels(neighbour_matrix(xy, float(eps)), int(min_pts))
    oct_ = np.zeros(n, np.int64) if octave is None else np.asarray(octave, np.int64).reshape(n)
    erase = oct_ == -5
    chosen = {}
    for i in range(n):
        cid = int(label[i])
        if cid > 0:
            if chosen.get(cid, 0) > features_from_cluster - 1:
                erase[i] = True
            else:
                chosen[cid] = chosen.get(cid, 0) + 1
    return np.flatnonzero(~erase).astype(np.int32)


def dbscan_bound(eps):
    """The least double s with (double)(float)sqrt(s) >= eps, by bisection over the bit patterns of the non-negative doubles
    (0 for eps <= 0 or NaN)."""
    eps = float(eps)
    if not eps > 0.0:
        return 0.0
    lo, hi = 0, 0x7FF0000000000000
    with np.errstate(all="ignore"):
        while lo < hi:
            mid = (lo + hi) // 2
            s = np.array([mid], np.uint64).view(np.float64)[0]
            if float(np.float32(np.sqrt(s))) >= eps:
                hi = mid
            else:
                lo = mid + 1
    return float(np.array([lo], np.uint64).view(np.float64)[0])
