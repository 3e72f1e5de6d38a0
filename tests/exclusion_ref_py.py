"""Sequential numpy restatement of the reference's three spatial-exclusion loops, the byte-for-byte yardstick of the GPU
exclusion filters (putslam_amd/csrc/ps_exclusion.h):

  choose_features_to_add_to_map   PUTSLAM::chooseFeaturesToAddToMap + removeCloseFeatures, src/PUTSLAM/PUTSLAM.cpp:53-178
  merge_tracked_features          Matcher::mergeTrackedFeatures, src/Matcher/matcher.cpp:97-130
  remove_too_close_features       Matcher::removeTooCloseFeatures, src/Matcher/matcher.cpp:886-974

The outer loops run in the reference's order, one candidate at a time; the innermost "for every existing feature" loop, which has
no side effect but its early return, is one numpy expression.  Every value is rounded where the reference rounds it (float32
differences, float32 or float64 sums, the real square root, the cast of the root) and compared with the threshold itself: the
squared-bound trick of the library is NOT used here.  Restated, not compiled: the reference files pull in all of Matcher and
PUTSLAM with OpenCV and Eigen."""
import numpy as np

F32, F64 = np.float32, np.float64


def _norm3_f32(p, q):
    """float norm = (tmp - feature3D).norm() on Eigen::Vector3f (PUTSLAM.cpp:61,84): float differences, squaredNorm summed as
    d0*d0 + (d1*d1 + d2*d2) (Eigen's 3-vector reduction, as tests/map_pairs_ref.py has it), sqrtf."""
    d = (p - q).astype(F32)
    s = (d[..., 0] * d[..., 0] + (d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])).astype(F32)
    return np.sqrt(s).astype(F32)


def _norm2_f64(p, q):
    """cv::norm(Point2f) = std::sqrt((double)x*x + (double)y*y) of the float difference."""
    d = (p - q).astype(F32).astype(F64)
    return np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])


def near_new_map(p3, p2, q3, q2, dE, dI):
    """removeCloseFeatures's two tests for existing (p3, p2) against candidate (q3, q2): float norm < double, (float)cv::norm <
    double (PUTSLAM.cpp:61-70)."""
    with np.errstate(invalid="ignore", over="ignore"):
        n3 = _norm3_f32(np.asarray(p3, F32), np.asarray(q3, F32)).astype(F64) < F64(dE)
        n2 = _norm2_f64(np.asarray(p2, F32), np.asarray(q2, F32)).astype(F32).astype(F64) < F64(dI)
    return n3 | n2


def near_merge(p2, q2, d):
    """cv::norm(a - b) < d, the double root (matcher.cpp:114-116)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return _norm2_f64(np.asarray(p2, F32), np.asarray(q2, F32)) < F64(d)


def near_too_close(p3, p2, q3, q2, a, b):
    """matcher.cpp:905-915: doubles of the float differences, sums left to right, double roots."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = (np.asarray(p3, F32) - np.asarray(q3, F32)).astype(F32).astype(F64)
        dist3 = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
        dist2 = _norm2_f64(np.asarray(p2, F32), np.asarray(q2, F32))
        return (dist3 < F64(a)) | (dist2 < F64(b))


def choose_features_to_add_to_map(feature3D, undistorted2D, map3, map2, added_counter, max_once, min_euclid, min_image):
    """PUTSLAM.cpp:98-178.  map3 / map2: the float casts of MapFeature::position and (u, v) (:58-60,66).  min_euclid / min_image
    arrive as float parameters (:101) and are compared as doubles (:62,68).  Returns (indices added, addedCounter)."""
    f3 = np.asarray(feature3D, F32).reshape(-1, 3)
    f2 = np.asarray(undistorted2D, F32).reshape(-1, 2)
    m3 = np.asarray(map3, F32).reshape(-1, 3)
    m2 = np.asarray(map2, F32).reshape(-1, 2)
    dE, dI = F64(F32(min_euclid)), F64(F32(min_image))
    add3 = np.zeros((len(f3), 3), F32)       # mapFeaturesToAdd: position = feature3D.cast<double>(), read back as float (:58-60)
    add2 = np.zeros((len(f3), 2), F32)
    added = []
    j = 0
    while j < len(f3) and added_counter < max_once:                                       # :112-114
        z = F64(f3[j, 2])
        if z > 0.8 and z < 6.0:                                                           # :117
            ok = not near_new_map(m3, m2, f3[j], f2[j], dE, dI).any()                     # :123-126
            if ok:
                k = len(added)
                ok = not near_new_map(add3[:k], add2[:k], f3[j], f2[j], dE, dI).any()     # :131-134
            if ok:
                k = len(added)
                add3[k] = f3[j].astype(F64).astype(F32)                                   # :163-169
                add2[k] = f2[j]
                added.append(j)
                added_counter += 1                                                        # :172
        j += 1
    return np.asarray(added, np.int32), added_counter


def merge_tracked_features(undistorted2D, sandbox2D, min_reproj):
    """matcher.cpp:97-130: the indices i of the sandbox features that are pushed back, in order."""
    have = np.asarray(undistorted2D, F32).reshape(-1, 2)
    sb = np.asarray(sandbox2D, F32).reshape(-1, 2)
    cur = np.zeros((len(have) + len(sb), 2), F32)
    cur[:len(have)] = have
    n = len(have)
    out = []
    for i in range(len(sb)):                                                              # :111
        if not near_merge(cur[:n], sb[i], min_reproj).any():                              # :113-120
            cur[n] = sb[i]                                                                # :122
            n += 1
            out.append(i)
    return np.asarray(out, np.int32)


def remove_too_close_features(features3D, undistorted2D, min_euclid, min_reproj):
    """matcher.cpp:900-919: featuresToRemove as an ascending int32 array."""
    f3 = np.asarray(features3D, F32).reshape(-1, 3)
    f2 = np.asarray(undistorted2D, F32).reshape(-1, 2)
    rm = np.zeros(len(f3), bool)
    for i in range(len(f3)):                                                              # :902
        rm[i + 1:] |= near_too_close(f3[i], f2[i], f3[i + 1:], f2[i + 1:], min_euclid, min_reproj)   # :903-917
    return np.flatnonzero(rm).astype(np.int32)


def erase_too_close(n, removed, match_train_idx):
    """matcher.cpp:921-963: what stays of the five per-feature vectors (positions, ascending) and of `matches` (positions whose
    trainIdx is not in featuresToRemove; the surviving matches are NOT renumbered)."""
    rm = set(int(x) for x in removed)
    stay = np.asarray([i for i in range(n) if i not in rm], np.int32)
    mstay = np.asarray([i for i, t in enumerate(match_train_idx) if int(t) not in rm], np.int32)
    return stay, mstay
