"""ctypes / numpy mirrors of the PODs in include/putslam_hip.h.

Field order and sizes follow the header exactly; tests/test_abi_layout.py checks
the sizes against the compiled library (ps_abi_sizeof_*).
"""
import ctypes as C

import numpy as np

PS_OK = 0
PS_DESC_BYTES = 32
PS_MAX_KPTS = 16384
PS_MAX_L2_DIM = 512

# RANSAC::ERROR_VERSION (reference include/putslam/TransformEst/RANSAC.h:22)
EUCLIDEAN_ERROR = 0
REPROJECTION_ERROR = 1
EUCLIDEAN_AND_REPROJECTION_ERROR = 2
MAHALANOBIS_ERROR = 3
ADAPTIVE_ERROR = 4

EST_RANSAC = 0
EST_USAC = 1
EST_FIXED = 2


class PsDMatch(C.Structure):
    _fields_ = [("queryIdx", C.c_int32), ("trainIdx", C.c_int32), ("imgIdx", C.c_int32),
                ("distance", C.c_float)]


class PsRansacParams(C.Structure):
    _fields_ = [("verbose", C.c_int32),
                ("errorVersion", C.c_int32), ("errorVersionVO", C.c_int32), ("errorVersionMap", C.c_int32),
                ("inlierThresholdEuclidean", C.c_double), ("inlierThresholdReprojection", C.c_double),
                ("inlierThresholdMahalanobis", C.c_double),
                ("minimalInlierRatioThreshold", C.c_double),
                ("minimalNumberOfMatches", C.c_int32), ("usedPairs", C.c_int32),
                ("iterationCount", C.c_int32)]


class PsRansacConfig(C.Structure):
    _fields_ = [("estimator", C.c_int32), ("numHypotheses", C.c_int32), ("seed", C.c_uint64),
                ("sampleIdx", C.POINTER(C.c_uint32))]


class PsRansacStats(C.Structure):
    _fields_ = [("numMatchesIn", C.c_int32), ("numMatchesValid", C.c_int32),
                ("bestHypothesis", C.c_int32), ("bestInlierCount", C.c_int32),
                ("iterationsRun", C.c_int32), ("numInliers", C.c_int32), ("accepted", C.c_int32),
                ("bestInlierRatio", C.c_float), ("pointInlierRatio", C.c_double)]


class PsFrameSet(C.Structure):
    _fields_ = [("desc", C.c_void_p), ("pts", C.c_void_p), ("nkpts", C.c_void_p),
                ("numFrames", C.c_int32), ("maxKpts", C.c_int32),
                ("descFrameStride", C.c_size_t), ("ptsFrameStride", C.c_size_t)]     # ABI 2: 0 = dense frames


class PsFrameSetF32(C.Structure):
    _fields_ = [("desc", C.c_void_p), ("pts", C.c_void_p), ("nkpts", C.c_void_p),
                ("numFrames", C.c_int32), ("maxKpts", C.c_int32), ("dim", C.c_int32),
                ("descRowStride", C.c_size_t), ("descFrameStride", C.c_size_t), ("ptsFrameStride", C.c_size_t)]   # 0 = dense


class PsPairResults(C.Structure):
    _fields_ = [("matches", C.c_void_p), ("numMatches", C.c_void_p), ("inlierMask", C.c_void_p),
                ("pose", C.c_void_p), ("stats", C.c_void_p)]


class PsMapBatch(C.Structure):
    _fields_ = [("maps", PsFrameSet), ("mapLevel", C.c_void_p), ("frames", PsFrameSet), ("curLevel", C.c_void_p),
                ("pairs", C.c_void_p), ("P", C.c_int32), ("maxMatches", C.c_int32), ("radiusBound", C.c_float),
                ("acceptRatio", C.c_double), ("radiusBoundPerPair", C.c_void_p), ("acceptRatioPerPair", C.c_void_p)]


class PsMapBatchF32(C.Structure):
    _fields_ = [("maps", PsFrameSetF32), ("mapLevel", C.c_void_p), ("frames", PsFrameSetF32), ("curLevel", C.c_void_p),
                ("pairs", C.c_void_p), ("P", C.c_int32), ("maxMatches", C.c_int32), ("radiusBound", C.c_float),
                ("acceptRatio", C.c_double), ("radiusBoundPerPair", C.c_void_p), ("acceptRatioPerPair", C.c_void_p)]


# PsExclusionRule forms and modes (include/putslam_hip.h)
PS_EXCL_NONE, PS_EXCL_F32, PS_EXCL_F64 = 0, 1, 2
PS_EXCL_GREEDY, PS_EXCL_ALL_EARLIER = 0, 1
PS_EXCL_MAX_CAND = 8192


class PsExclusionRule(C.Structure):
    _fields_ = [("bound3", C.c_double), ("bound2", C.c_double), ("depthMin", C.c_double), ("depthMax", C.c_double),
                ("form3", C.c_int32), ("form2", C.c_int32), ("mode", C.c_int32), ("maxKeep", C.c_int32),
                ("depthGate", C.c_int32), ("reserved", C.c_int32)]


# ps_map_views_device (include/putslam_hip.h): the resident feature map, the request and the output block
PS_VIEW_REQUIRE_VISIBLE = 1
PS_LEVEL_OCTAVE_MIN, PS_LEVEL_OCTAVE_MAX = -16, 47
PS_VIEW_INVALID = -2 ** 31      # viewCount of a view with a bad count, index, pose id or octave


class PsMapStore(C.Structure):
    _fields_ = [("pos", C.c_void_p), ("obsStart", C.c_void_p), ("obsPose", C.c_void_p), ("obsDesc", C.c_void_p),
                ("obsOctave", C.c_void_p), ("obsDetDist", C.c_void_p),
                ("numFeatures", C.c_int32), ("numObs", C.c_int32), ("numPoses", C.c_int32), ("reserved", C.c_int32)]


class PsMapViewRequest(C.Structure):
    _fields_ = [("camInv", C.c_void_p), ("poseAngle", C.c_void_p), ("cand", C.c_void_p), ("candCounts", C.c_void_p),
                ("maxAngle", C.c_double), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("imageW", C.c_double), ("imageH", C.c_double),
                ("V", C.c_int32), ("candCapacity", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


class PsMapViewOut(C.Structure):
    _fields_ = [("views", PsFrameSet), ("mapLevel", C.c_void_p), ("viewCount", C.c_void_p), ("featIdx", C.c_void_p),
                ("obsIdx", C.c_void_p), ("posCam", C.c_void_p), ("uv", C.c_void_p), ("angle", C.c_void_p)]


# ps_pose_sets_device / ps_loop_pairs_device (include/putslam_hip.h): loop-closure candidates from the resident store
PS_LOOP_MAX_SETS = 1024
PS_SET_INVALID = -2 ** 31       # setCount of a set with a bad pose id (or of every set of a store with a bad range); numPaired of
                                # a candidate that names such a set


class PsPoseSetRequest(C.Structure):
    _fields_ = [("obsPoint3D", C.c_void_p), ("poses", C.c_void_p), ("S", C.c_int32), ("reserved", C.c_int32)]


class PsPoseSetOut(C.Structure):
    _fields_ = [("sets", PsFrameSet), ("setCount", C.c_void_p), ("featIdx", C.c_void_p), ("obsIdx", C.c_void_p)]


class PsLoopBatch(C.Structure):
    _fields_ = [("sets", PsFrameSet), ("setCount", C.c_void_p), ("featIdx", C.c_void_p), ("pairs", C.c_void_p),
                ("L", C.c_int32), ("S", C.c_int32), ("minNumberOfFeaturesLC", C.c_int32), ("reserved", C.c_int32),
                ("matchingRatioThresholdLC", C.c_double)]


class PsLoopResults(C.Structure):
    _fields_ = [("pair", PsPairResults), ("ratio", C.c_void_p), ("closed", C.c_void_p), ("numPaired", C.c_void_p),
                ("pairedRows", C.c_void_p), ("pairedFeat", C.c_void_p)]


# The resident store with float descriptor rows (include/putslam_hip.h)
class PsMapStoreF32(C.Structure):
    _fields_ = [("pos", C.c_void_p), ("obsStart", C.c_void_p), ("obsPose", C.c_void_p), ("obsDesc", C.c_void_p),
                ("obsOctave", C.c_void_p), ("obsDetDist", C.c_void_p),
                ("numFeatures", C.c_int32), ("numObs", C.c_int32), ("numPoses", C.c_int32), ("dim", C.c_int32),
                ("obsDescRowStride", C.c_size_t)]


class PsMapViewOutF32(C.Structure):
    _fields_ = [("views", PsFrameSetF32), ("mapLevel", C.c_void_p), ("viewCount", C.c_void_p), ("featIdx", C.c_void_p),
                ("obsIdx", C.c_void_p), ("posCam", C.c_void_p), ("uv", C.c_void_p), ("angle", C.c_void_p)]


class PsPoseSetOutF32(C.Structure):
    _fields_ = [("sets", PsFrameSetF32), ("setCount", C.c_void_p), ("featIdx", C.c_void_p), ("obsIdx", C.c_void_p)]


class PsLoopBatchF32(C.Structure):
    _fields_ = [("sets", PsFrameSetF32), ("setCount", C.c_void_p), ("featIdx", C.c_void_p), ("pairs", C.c_void_p),
                ("L", C.c_int32), ("S", C.c_int32), ("minNumberOfFeaturesLC", C.c_int32), ("reserved", C.c_int32),
                ("matchingRatioThresholdLC", C.c_double)]


# Pyramidal Lucas-Kanade tracking (include/putslam_hip.h)
PS_KLT_USE_INITIAL_FLOW = 4
PS_KLT_GET_MIN_EIGENVALS = 8


class PsKltParams(C.Structure):
    _fields_ = [("eps", C.c_double), ("minEigThreshold", C.c_double), ("winSize", C.c_int32), ("maxLevels", C.c_int32),
                ("maxCount", C.c_int32), ("flags", C.c_int32)]


class PsImageSet(C.Structure):
    _fields_ = [("pixels", C.c_void_p), ("rowStride", C.c_size_t), ("frameStride", C.c_size_t), ("numFrames", C.c_int32),
                ("rows", C.c_int32), ("cols", C.c_int32), ("channels", C.c_int32)]


def klt_params(win_size=7, max_levels=3, max_count=30, eps=0.01, flags=0, min_eig_threshold=1e-4):
    """PsKltParams; the defaults are the shipped OpenCVParams (winSize 7, maxLevels 3, maxIter 30, eps 0.01)."""
    return PsKltParams(float(eps), float(min_eig_threshold), int(win_size), int(max_levels), int(max_count), int(flags))


# FAST-9/16 key point detection (include/putslam_hip.h)
class PsDetectParams(C.Structure):
    _fields_ = [("threshold", C.c_int32), ("nonmaxSuppression", C.c_int32), ("gridRows", C.c_int32), ("gridCols", C.c_int32),
                ("maximalTrackedFeatures", C.c_int32), ("reserved", C.c_int32)]


def detect_params(threshold=10, nonmax_suppression=True, grid_rows=1, grid_cols=1, maximal_tracked_features=500):
    """PsDetectParams; the defaults are cv::FastFeatureDetector::create()'s (threshold 10, suppression on) and the shipped
    OpenCVParams (gridRows = gridCols = 1, maximalTrackedFeatures 500)."""
    return PsDetectParams(int(threshold), 1 if nonmax_suppression else 0, int(grid_rows), int(grid_cols),
                          int(maximal_tracked_features), 0)


# ORB descriptor extraction (include/putslam_hip.h)
class PsOrbParams(C.Structure):
    _fields_ = [("scaleFactor", C.c_float), ("nLevels", C.c_int32), ("reserved", C.c_int32 * 2)]


def orb_params(scale_factor=1.2, n_levels=8):
    """PsOrbParams; the defaults are cv::ORB::create()'s (scaleFactor 1.2f, 8 levels)."""
    return PsOrbParams(float(scale_factor), int(n_levels), (C.c_int32 * 2)(0, 0))


# ORB key point detection (include/putslam_hip.h)
class PsOrbDetectParams(C.Structure):
    _fields_ = [("nFeatures", C.c_int32), ("scaleFactor", C.c_float), ("nLevels", C.c_int32), ("fastThreshold", C.c_int32),
                ("gridRows", C.c_int32), ("gridCols", C.c_int32), ("maximalTrackedFeatures", C.c_int32), ("reserved", C.c_int32)]


def orb_detect_params(n_features=500, scale_factor=1.2, n_levels=8, fast_threshold=20, grid_rows=1, grid_cols=1,
                      maximal_tracked_features=500):
    """PsOrbDetectParams; the defaults are cv::ORB::create()'s (500 features, scaleFactor 1.2f, 8 levels, fastThreshold 20) and the
    shipped OpenCVParams (gridRows = gridCols = 1, maximalTrackedFeatures 500)."""
    return PsOrbDetectParams(int(n_features), float(scale_factor), int(n_levels), int(fast_threshold), int(grid_rows), int(grid_cols),
                             int(maximal_tracked_features), 0)


# Frame assembly and the front end (include/putslam_hip.h)
class PsDepthSet(C.Structure):
    _fields_ = [("pixels", C.c_void_p), ("rowStride", C.c_size_t), ("frameStride", C.c_size_t), ("numFrames", C.c_int32),
                ("rows", C.c_int32), ("cols", C.c_int32)]


class PsFrameGeometry(C.Structure):
    _fields_ = [("K", C.c_float * 9), ("dist5", C.c_double * 5), ("depthImageScale", C.c_double)]


class PsFrameRowsOut(C.Structure):
    _fields_ = [("pts", C.c_void_p), ("nkpts", C.c_void_p), ("xy", C.c_void_p), ("xyUndist", C.c_void_p), ("angle", C.c_void_p),
                ("response", C.c_void_p), ("octave", C.c_void_p), ("srcIdx", C.c_void_p), ("detDist", C.c_void_p),
                ("angleIn", C.c_void_p), ("responseIn", C.c_void_p), ("octaveIn", C.c_void_p)]


class PsFrontEndParams(C.Structure):
    _fields_ = [("detect", PsOrbDetectParams), ("describe", PsOrbParams), ("DBScanEps", C.c_double)]


def frame_geometry(K, dist5=(0.0,) * 5, depth_image_scale=5000.0):
    """PsFrameGeometry: K nine floats row-major, dist5 (k1, k2, p1, p2, k3), depthImageScale."""
    K = np.asarray(K, np.float32).reshape(9)
    d = np.asarray(dist5, np.float64).reshape(5)
    return PsFrameGeometry((C.c_float * 9)(*K.tolist()), (C.c_double * 5)(*d.tolist()), float(depth_image_scale))


def front_end_params(detect=None, describe=None, dbscan_eps=10.0):
    """PsFrontEndParams: detect _abi.orb_detect_params(...) and describe _abi.orb_params(...), default the shipped ones (which
    share scaleFactor and nLevels, as the front end requires); dbscan_eps OpenCVParams.DBScanEps."""
    detect = detect or orb_detect_params()
    describe = describe or orb_params(detect.scaleFactor, detect.nLevels)
    return PsFrontEndParams(detect, describe, float(dbscan_eps))


# The tracking VO step (include/putslam_hip.h)
class PsPointSets(C.Structure):
    _fields_ = [("pts", C.c_void_p), ("counts", C.c_void_p), ("numSets", C.c_int32), ("capacity", C.c_int32), ("setStride", C.c_size_t)]


class PsTrackedCarry(C.Structure):
    _fields_ = [("angle", C.c_void_p), ("response", C.c_void_p), ("octave", C.c_void_p), ("detDist", C.c_void_p)]


class PsTrackedRows(C.Structure):
    _fields_ = [("xy", C.c_void_p), ("xyUndist", C.c_void_p), ("pts", C.c_void_p), ("counts", C.c_void_p), ("angle", C.c_void_p),
                ("response", C.c_void_p), ("octave", C.c_void_p), ("detDist", C.c_void_p)]


class PsTrackVoParams(C.Structure):
    _fields_ = [("trackingErrorThreshold", C.c_double), ("minimalReprojDistanceNewTrackingFeatures", C.c_double),
                ("removeTooCloseFeatures", C.c_int32), ("reserved", C.c_int32)]


class PsTrackVoIn(C.Structure):
    _fields_ = [("pairs", C.c_void_p), ("depthFrame", C.c_void_p), ("prevXY", C.c_void_p), ("prevPts", C.c_void_p),
                ("prevCounts", C.c_void_p), ("prev", PsTrackedCarry)]


class PsTrackVoOut(C.Structure):
    _fields_ = [("nextPts", C.c_void_p), ("status", C.c_void_p), ("err", C.c_void_p), ("matches", C.c_void_p),
                ("numMatches", C.c_void_p), ("keptIdx", C.c_void_p), ("rows", PsTrackedRows), ("inlierMask", C.c_void_p),
                ("pose", C.c_void_p), ("stats", C.c_void_p)]


def track_vo_params(tracking_error_threshold=25.0, min_reproj_distance=3.0, remove_too_close_features=0):
    """PsTrackVoParams; the defaults are the shipped OpenCVParams (trackingErrorThreshold 25, minimalReprojDistanceNewTrackingFeatures
    3, removeTooCloseFeatures 0 -- the only value ps_track_vo_pairs takes)."""
    return PsTrackVoParams(float(tracking_error_threshold), float(min_reproj_distance), int(remove_too_close_features), 0)


# Closing the tracking VO step (include/putslam_hip.h)
class PsTrackCandidates(C.Structure):
    _fields_ = [("xy", C.c_void_p), ("xyUndist", C.c_void_p), ("pts", C.c_void_p), ("angle", C.c_void_p), ("response", C.c_void_p),
                ("octave", C.c_void_p), ("detDist", C.c_void_p), ("counts", C.c_void_p), ("numFrames", C.c_int32), ("capacity", C.c_int32)]


class PsTrackCloseParams(C.Structure):
    _fields_ = [("minimalReprojDistanceNewTrackingFeatures", C.c_double), ("minimalTrackedFeatures", C.c_int32),
                ("removeTooCloseFeatures", C.c_int32)]


class PsTrackCloseOut(C.Structure):
    _fields_ = [("desc", C.c_void_p), ("rows", PsTrackedRows), ("srcIdx", C.c_void_p), ("refill", C.c_void_p)]


def track_close_params(minimal_tracked_features=150, min_reproj_distance=3.0, remove_too_close_features=0):
    """PsTrackCloseParams; the defaults are the shipped OpenCVParams (minimalTrackedFeatures 150,
    minimalReprojDistanceNewTrackingFeatures 3, removeTooCloseFeatures 0 -- the only value ps_track_close_pairs takes)."""
    return PsTrackCloseParams(float(min_reproj_distance), int(minimal_tracked_features), int(remove_too_close_features))


# Measurement uncertainty (include/putslam_hip.h)
UNCERTAINTY_OFF, UNCERTAINTY_IMAGE_COORDINATES, UNCERTAINTY_NORMAL, UNCERTAINTY_RGB_GRADIENT = -1, 0, 1, 2
NAN_BITS = 0x7FF8000000000000     # the one NaN the uncertainty kernels write


class PsSensorModel(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("fu", "fv", "cu", "cv", "varU", "varV", "c3", "c2", "c1", "c0", "scaleUncertaintyNormal",
                                          "scaleUncertaintyGradient")]


class PsUncertaintyOut(C.Structure):
    _fields_ = [("normal", C.c_void_p), ("gradient", C.c_void_p), ("info", C.c_void_p)]


class PsMeasurementEdgesOut(C.Structure):
    _fields_ = [("count", C.c_void_p), ("mapRow", C.c_void_p), ("curRow", C.c_void_p), ("uv", C.c_void_p), ("position", C.c_void_p),
                ("normal", C.c_void_p), ("gradient", C.c_void_p), ("info", C.c_void_p)]


def sensor_model(**fields):
    """PsSensorModel: DepthSensorModel::Config()'s defaults (ps_sensor_model_default's numbers; the two scale factors 0, which the
    reference leaves unset) with the named fields replaced."""
    s = PsSensorModel(582.64, 586.97, 320.17, 260.0, 1.1046, 0.64160, -8.9997e-06, 3.069e-003, 3.6512e-006, -0.0017512e-3, 0.0, 0.0)
    for k, v in fields.items():
        assert hasattr(s, k), k
        setattr(s, k, float(v))
    return s


# Sub-pixel matching on patches (include/putslam_hip.h)
PATCH_MAX_ITERATIONS, PATCH_CONVERGED, PATCH_NAN_HESSIAN, PATCH_OUT_OF_IMAGE, PATCH_MOVED_TOO_FAR = 0, 1, 2, 3, 4
PATCH_OLD_TAPS_OUTSIDE, PATCH_NEW_TAPS_OUTSIDE = 5, 6
PATCH_GIVEN_MODEL = 1


class PsPatchParams(C.Structure):
    _fields_ = [("minSqrtIncrement", C.c_double), ("patchSize", C.c_int32), ("maxIter", C.c_int32), ("flags", C.c_int32),
                ("reserved", C.c_int32)]


class PsPatchModel(C.Structure):
    _fields_ = [("patch", C.c_void_p), ("gx", C.c_void_p), ("gy", C.c_void_p), ("invHessian", C.c_void_p)]


def patch_params(patch_size=13, max_iter=50, min_sqrt_increment=0.04, flags=0):
    """PsPatchParams; the defaults are the shipped PatchesParams (patchSize 13, maxIterationCount 50, minSqrtError 0.04)."""
    return PsPatchParams(float(min_sqrt_increment), int(patch_size), int(max_iter), int(flags), 0)


class PsHostPairResults(C.Structure):
    _fields_ = [("matches", C.c_void_p), ("numMatches", C.c_void_p), ("inlierMask", C.c_void_p),
                ("pose", C.c_void_p), ("stats", C.c_void_p), ("firstPair", C.c_int64), ("count", C.c_int32),
                ("maxKpts", C.c_int32), ("epoch", C.c_int32), ("resultMode", C.c_int32)]


PS_ERR_BUSY = -6

DMATCH_DTYPE = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])
STATS_DTYPE = np.dtype([("numMatchesIn", "<i4"), ("numMatchesValid", "<i4"), ("bestHypothesis", "<i4"),
                        ("bestInlierCount", "<i4"), ("iterationsRun", "<i4"), ("numInliers", "<i4"),
                        ("accepted", "<i4"), ("bestInlierRatio", "<f4"), ("pointInlierRatio", "<f8")])
assert DMATCH_DTYPE.itemsize == C.sizeof(PsDMatch) == 16
assert STATS_DTYPE.itemsize == C.sizeof(PsRansacStats) == 40

# Camera intrinsics of the reference's default dataset config
# (resources/datasetConfig/freiburg1_desk.xml:5-6,20; the same constants are hard-coded at RGBD.cpp:22-23).
TUM_FR1_K = np.array([517.3, 0.0, 318.6, 0.0, 516.5, 255.3, 0.0, 0.0, 1.0], dtype=np.float32)
TUM_DEPTH_SCALE = 5000.0
# rgbDistortion (k1, k2, p1, p2, k3) of the same file, :7 -- what RGBD::removeImageDistortion is given (RGBD.cpp:254-314)
TUM_FR1_DIST = (-0.0410, 0.3286, 0.0087, 0.0051, -0.5643)


def default_ransac_params(error_version=EUCLIDEAN_ERROR, lc=False):
    """Shipped defaults: resources/putslammatcherOpenCVParameters.xml:29-37 (LC variant: ...LC.xml:30)."""
    p = PsRansacParams()
    p.verbose = 0
    p.errorVersion = error_version
    p.errorVersionVO = 0
    p.errorVersionMap = 0
    p.inlierThresholdEuclidean = 0.04
    p.inlierThresholdReprojection = 2.0
    p.inlierThresholdMahalanobis = 0.0002
    p.minimalInlierRatioThreshold = 0.15 if lc else 0.2
    p.minimalNumberOfMatches = 10 if lc else 15
    p.usedPairs = 3
    p.iterationCount = 0
    return p


def make_config(estimator=EST_RANSAC, num_hypotheses=487, seed=1, sample_idx=None):
    """Returns (cfg, keepalive). sample_idx: optional (H,3) uint32 array of raw draws."""
    cfg = PsRansacConfig()
    cfg.estimator = estimator
    cfg.numHypotheses = int(num_hypotheses)
    cfg.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    keep = None
    if sample_idx is not None:
        keep = np.ascontiguousarray(sample_idx, dtype=np.uint32)
        assert keep.shape == (cfg.numHypotheses, 3)
        cfg.sampleIdx = keep.ctypes.data_as(C.POINTER(C.c_uint32))
    else:
        cfg.sampleIdx = None
    return cfg, keep
