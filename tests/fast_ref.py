"""MatcherOpenCV::detectFeatures for detector = "FAST" (reference src/Matcher/matcherOpenCV.cpp:118-180), restated twice in numpy
from the project's reading of OpenCV 3.x's fast.cpp / fast_score.cpp and of the 8-bit cvtColor(RGB2GRAY).
The two restatements share the ring and nothing else:

 (a) literal      the detector as a sequential program: the row loop with the 512-entry threshold table, the quick rejections on
                  the antipodal pairs, the consecutive-count loop over the ring repeated to 25 entries, the score by pairwise min /
                  max over the even arcs with its early `continue`, the three row buffers of the suppression that emit row i-1
                  while row i is scored; then the grid loop, ordering each list with a stable sort;
 (b) closed form  d = v - ring as a (16, rows, cols) stack, the arcs of nine as min / max over rolled stacks, corner = max(D, B) > t,
                  score = max(t, D, B) - 1, suppression by comparing with the eight shifted maps, and the final order as ONE
                  lexicographic key (response descending, ROI in loop order, raster position) with the per-ROI cut counted by rank.

tests/test_fast_ref_host.py holds them to each other; the GPU tests hold the library to them byte for byte.
Both orderings are STABLE by this project's definition (the reference's std::sort is not)."""
import numpy as np

# (dx, dy) of ring pixel k; y grows downwards
RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1),
        (-2, 2), (-1, 3)]


def to_gray(img):
    """(rows, cols) uint8 of an image (rows, cols) -- taken as grey already -- or (rows, cols, 3): channel 0 gets the red weight."""
    img = np.asarray(img, np.uint8)
    if img.ndim == 2:
        return img.copy()
    c = img.astype(np.int64)
    return ((c[..., 0] * 4899 + c[..., 1] * 9617 + c[..., 2] * 1868 + 8192) >> 14).astype(np.uint8)


def clamp_threshold(threshold):
    return min(max(int(threshold), 0), 255)


# ---------------------------------------------------------------------------------------------- (a) literal
def _corner_score_literal(img, y, x, t):
    v = img[y][x]
    d = [v - img[y + RING[k & 15][1]][x + RING[k & 15][0]] for k in range(25)]
    a0 = t
    for k in range(0, 16, 2):
        a = min(d[k + 1], d[k + 2])
        a = min(a, d[k + 3])
        if a <= a0:
            continue
        a = min(a, d[k + 4])
        a = min(a, d[k + 5])
        a = min(a, d[k + 6])
        a = min(a, d[k + 7])
        a = min(a, d[k + 8])
        a0 = max(a0, min(a, d[k]))
        a0 = max(a0, min(a, d[k + 9]))
    b0 = -a0
    for k in range(0, 16, 2):
        b = max(d[k + 1], d[k + 2])
        b = max(b, d[k + 3])
        b = max(b, d[k + 4])
        b = max(b, d[k + 5])
        if b >= b0:
            continue
        b = max(b, d[k + 6])
        b = max(b, d[k + 7])
        b = max(b, d[k + 8])
        b0 = min(b0, max(b, d[k]))
        b0 = min(b0, max(b, d[k + 9]))
    return -b0 - 1


def fast_literal(gray, t, nms=True):
    """FAST-9/16 on one image (an ROI is an image of its own).  Returns (corner (rows, cols) uint8, score (rows, cols) uint8 --
    zeros when nms is off, as no score is computed then --, key points [(x, y, response)] in emission order)."""
    gray = np.asarray(gray, np.uint8)
    R, C = gray.shape
    img = gray.tolist()
    tab = [1 if i < -t else (2 if i > t else 0) for i in range(-255, 256)]
    corner, score = np.zeros((R, C), np.uint8), np.zeros((R, C), np.uint8)
    buf = [[0] * C for _ in range(3)]
    cpbuf = [[] for _ in range(3)]
    kps = []
    for i in range(3, R - 2):
        curr = buf[(i - 3) % 3]
        for j in range(C):
            curr[j] = 0
        cornerpos = cpbuf[(i - 3) % 3]
        del cornerpos[:]
        if i < R - 3:
            for j in range(3, C - 3):
                v = img[i][j]
                o = 255 - v     # tab[o + ring]: 1 = the ring pixel is darker than v - t, 2 = brighter than v + t
                r = [img[i + dy][j + dx] for dx, dy in RING]
                d = tab[o + r[0]] | tab[o + r[8]]
                if d == 0:
                    continue
                d &= tab[o + r[2]] | tab[o + r[10]]
                d &= tab[o + r[4]] | tab[o + r[12]]
                d &= tab[o + r[6]] | tab[o + r[14]]
                if d == 0:
                    continue
                d &= tab[o + r[1]] | tab[o + r[9]]
                d &= tab[o + r[3]] | tab[o + r[11]]
                d &= tab[o + r[5]] | tab[o + r[13]]
                d &= tab[o + r[7]] | tab[o + r[15]]
                found = False
                if d & 1:
                    vt, count = v - t, 0
                    for k in range(25):
                        if r[k & 15] < vt:
                            count += 1
                            if count > 8:
                                found = True
                                break
                        else:
                            count = 0
                if d & 2 and not found:
                    vt, count = v + t, 0
                    for k in range(25):
                        if r[k & 15] > vt:
                            count += 1
                            if count > 8:
                                found = True
                                break
                        else:
                            count = 0
                if found:
                    cornerpos.append(j)
                    corner[i, j] = 1
                    if nms:
                        curr[j] = _corner_score_literal(img, i, j, t)
                        score[i, j] = curr[j]
        if i == 3:
            continue
        prev, pprev = buf[(i - 4) % 3], buf[(i - 5) % 3]
        for j in cpbuf[(i - 4) % 3]:
            s = prev[j]
            if not nms or (s > prev[j + 1] and s > prev[j - 1] and s > pprev[j - 1] and s > pprev[j] and s > pprev[j + 1]
                           and s > curr[j - 1] and s > curr[j] and s > curr[j + 1]):
                kps.append((j, i - 1, s))
    return corner, score, kps


def roi_rects(rows, cols, grid_rows, grid_cols):
    """[(x0, y0, w, h)] in the order of the reference's loop: columns outer, rows inner; integer divisions."""
    return [(k * cols // grid_cols, i * rows // grid_rows, cols // grid_cols, rows // grid_rows)
            for k in range(grid_cols) for i in range(grid_rows)]


def max_in_roi(max_features, grid_rows, grid_cols):
    return (max_features * 3) // (grid_cols * grid_rows)


def _pack(kps):
    xy = np.array([[k[0], k[1]] for k in kps], np.float32).reshape(-1, 2)
    return xy, np.array([k[2] for k in kps], np.float32)


def detect_literal(img, threshold=10, nms=True, grid_rows=1, grid_cols=1, max_features=500):
    """The grid loop of detectFeatures around fast_literal.  Returns (xy (n, 2) float32, response (n,) float32)."""
    gray = to_gray(img)
    t = clamp_threshold(threshold)
    per_roi = max_in_roi(max_features, grid_rows, grid_cols)
    raw = []
    for x0, y0, w, h in roi_rects(gray.shape[0], gray.shape[1], grid_rows, grid_cols):
        kps = fast_literal(gray[y0:y0 + h, x0:x0 + w], t, nms)[2]
        order = np.argsort(-np.array([k[2] for k in kps], np.int64), kind="stable")
        for j in order[:per_roi]:
            raw.append((np.float32(kps[j][0]) + np.float32(x0), np.float32(kps[j][1]) + np.float32(y0), kps[j][2]))
    order = np.argsort(-np.array([k[2] for k in raw], np.int64), kind="stable")
    return _pack([raw[j] for j in order[:max_features]])


# ---------------------------------------------------------------------------------------------- (b) closed form
def fast_closed(gray, t):
    """(corner, score) maps of one image: arcs of nine by min / max over rolled stacks.  The score is there whatever the mode."""
    g = np.asarray(gray, np.uint8).astype(np.int32)
    R, C = g.shape
    corner, score = np.zeros((R, C), np.uint8), np.zeros((R, C), np.uint8)
    if R < 7 or C < 7:
        return corner, score
    v = g[3:R - 3, 3:C - 3]
    d = np.stack([v - g[3 + dy:R - 3 + dy, 3 + dx:C - 3 + dx] for dx, dy in RING])
    D = np.max(np.stack([np.min(np.roll(d, -s, axis=0)[:9], axis=0) for s in range(16)]), axis=0)
    B = np.max(np.stack([np.min(np.roll(-d, -s, axis=0)[:9], axis=0) for s in range(16)]), axis=0)
    m = np.maximum(D, B)
    is_corner = m > t
    corner[3:R - 3, 3:C - 3] = is_corner
    score[3:R - 3, 3:C - 3] = np.where(is_corner, np.maximum(m, t) - 1, 0)
    return corner, score


def emitted_closed(corner, score, nms):
    """(mask of the emitted pixels, their response map) of one image."""
    if not nms:
        return corner.astype(bool), np.zeros_like(score)
    p = np.pad(score.astype(np.int32), 1)
    R, C = score.shape
    nb = np.max(np.stack([p[1 + dy:1 + dy + R, 1 + dx:1 + dx + C] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0)]), axis=0)
    return corner.astype(bool) & (score.astype(np.int32) > nb), score


def maps_closed(img, threshold, grid_rows=1, grid_cols=1):
    """(grey, score, corner) of the whole image with every ROI scored as an image of its own: what ps_debug_fast_maps returns."""
    gray = to_gray(img)
    t = clamp_threshold(threshold)
    score, corner = np.zeros_like(gray), np.zeros_like(gray)
    for x0, y0, w, h in roi_rects(gray.shape[0], gray.shape[1], grid_rows, grid_cols):
        c, s = fast_closed(gray[y0:y0 + h, x0:x0 + w], t)
        corner[y0:y0 + h, x0:x0 + w], score[y0:y0 + h, x0:x0 + w] = c, s
    return gray, score, corner


def detect_closed(img, threshold=10, nms=True, grid_rows=1, grid_cols=1, max_features=500):
    """detectFeatures as one ordering: every emitted pixel gets (response, ROI number, raster position); the per-ROI cut keeps the
    ranks below maxInROI inside each ROI, the final order is response descending, then ROI, then raster position."""
    gray = to_gray(img)
    t = clamp_threshold(threshold)
    per_roi = max_in_roi(max_features, grid_rows, grid_cols)
    xs, ys, rs, qs = [], [], [], []
    for q, (x0, y0, w, h) in enumerate(roi_rects(gray.shape[0], gray.shape[1], grid_rows, grid_cols)):
        c, s = fast_closed(gray[y0:y0 + h, x0:x0 + w], t)
        mask, resp = emitted_closed(c, s, nms)
        y, x = np.nonzero(mask)              # raster order
        r = resp[y, x].astype(np.int64)
        rank = np.empty(len(r), np.int64)    # place inside the ROI: response descending, raster order among equals
        rank[np.lexsort((np.arange(len(r)), -r))] = np.arange(len(r))
        keep = rank < per_roi
        xs.append(x[keep] + x0)
        ys.append(y[keep] + y0)
        rs.append(r[keep])
        qs.append(np.full(int(keep.sum()), q, np.int64))
    x, y, r, q = (np.concatenate(a) if a else np.zeros(0, np.int64) for a in (xs, ys, rs, qs))
    order = np.lexsort((x, y, q, -r))[:max_features]    # inside one ROI raster order is (y, x)
    return np.stack([x[order], y[order]], axis=1).astype(np.float32).reshape(-1, 2), r[order].astype(np.float32)


# ---------------------------------------------------------------------------------------------- scenes
def blocks(rows, cols, seed, n, noise=0):
    """n random rectangles of random grey on grey 100, optionally with uniform noise of +-noise."""
    rng = np.random.RandomState(seed)
    img = np.full((rows, cols), 100, np.int32)
    for _ in range(n):
        x0, y0 = rng.randint(0, cols), rng.randint(0, rows)
        w, h = rng.randint(2, max(3, cols // 4)), rng.randint(2, max(3, rows // 4))
        img[y0:y0 + h, x0:x0 + w] = rng.randint(0, 256)
    if noise:
        img = img + rng.randint(-noise, noise + 1, size=img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def noise256(rows, cols, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(rows, cols)).astype(np.uint8)


def noise4(rows, cols, seed):
    """Noise of four levels: the scores are few, so most key points tie."""
    return np.array([20, 80, 140, 200], np.uint8)[np.random.RandomState(seed).randint(0, 4, size=(rows, cols))]


def colour(gray_like, seed):
    """A three-channel image whose channels differ (so that the grey weights matter): the scene plus two decorrelated channels."""
    rng = np.random.RandomState(seed)
    g = np.asarray(gray_like, np.uint8)
    return np.stack([g, np.roll(g, 3, axis=1) ^ rng.randint(0, 64, size=g.shape).astype(np.uint8), np.flipud(g)], axis=2)


SCENES = {
    "blocks": lambda rows, cols: blocks(rows, cols, 3, max(8, rows * cols // 100), noise=6),
    "noise256": lambda rows, cols: noise256(rows, cols, 7),
    "noise4": lambda rows, cols: noise4(rows, cols, 5),
}
