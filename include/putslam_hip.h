/* putslam_hip.h -- C ABI of the MI355X-native PUTSLAM visual-odometry front end.
 *
 * One data-parallel path of LRMPUT/PUTSLAM, hand-written for gfx950 (CDNA4):
 *   brute-force 256-bit Hamming matching with OpenCV cross-check semantics
 *   -> depth filter -> 3-point RANSAC / USAC with a float Umeyama fit
 *   -> inlier scoring (Euclidean / reprojection) -> refit -> acceptance gate,
 * plus the double-precision N-point Kabsch fit behind TransformEst and the
 * pinhole back-projection helper.
 *
 * Every entry point names the reference interface (file:line under the
 * PUTSLAM tree) it replaces.  Signatures are plain C: pointers, sizes, PODs.
 * All functions return PS_OK (0) or a negative PsStatus; on failure the
 * reference's own fallback outputs (identity pose, zero inliers) are still
 * written, because the reference path has no exceptions and no error codes
 * (src/TransformEst/RANSAC.cpp:77-80,161-164,239-242).
 *
 * There is NO CPU fallback behind this ABI.  If no HIP device is usable the
 * context constructor fails with PS_ERR_NO_DEVICE and every call fails loudly.
 */
#ifndef PUTSLAM_HIP_H_
#define PUTSLAM_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PS_ABI_VERSION 2          /* 2: PsFrameSet carries frame strides (packed frames) */
#define PS_DESC_BYTES 32          /* ORB (matcherOpenCV.cpp:90) and LDB (ldb.cpp:61,657) rows: 256 bit */
#define PS_MAX_KPTS 16384         /* keypoints per frame handled by one launch (LDS-resident cross-check) */
#define PS_MAX_HYPOTHESES (1 << 20)

typedef enum PsStatus {
    PS_OK = 0,
    PS_ERR_BAD_ARG = -1,
    PS_ERR_NO_DEVICE = -2,
    PS_ERR_HIP = -3,
    PS_ERR_ALLOC = -4,
    PS_ERR_UNSUPPORTED = -5,
    PS_ERR_BUSY = -6            /* pipelined streaming: every lane holds results the caller has not popped yet */
} PsStatus;

/* cv::DMatch: same field order and size (16 B) as OpenCV's struct, so a
 * std::vector<cv::DMatch>::data() can be passed straight through. */
typedef struct PsDMatch {
    int32_t queryIdx;   /* row of the PREVIOUS frame's descriptors (matcher.cpp:470-471) */
    int32_t trainIdx;   /* row of the CURRENT frame's descriptors */
    int32_t imgIdx;     /* always 0 */
    float distance;     /* integer Hamming distance 0..256 as float */
} PsDMatch;

/* RANSAC::ERROR_VERSION, include/putslam/TransformEst/RANSAC.h:22 */
typedef enum PsErrorVersion {
    PS_EUCLIDEAN_ERROR = 0,
    PS_REPROJECTION_ERROR = 1,
    PS_EUCLIDEAN_AND_REPROJECTION_ERROR = 2,
    PS_MAHALANOBIS_ERROR = 3,  /* dead in the reference (cov never set, RANSAC.cpp:301-303): scores 0 */
    PS_ADAPTIVE_ERROR = 4
} PsErrorVersion;

/* RANSAC::parameters, include/putslam/TransformEst/RANSAC.h:23-31 (same fields, same order). */
typedef struct PsRansacParams {
    int32_t verbose;
    int32_t errorVersion, errorVersionVO, errorVersionMap;
    double inlierThresholdEuclidean, inlierThresholdReprojection, inlierThresholdMahalanobis;
    double minimalInlierRatioThreshold;
    int32_t minimalNumberOfMatches;
    int32_t usedPairs;        /* only 3 is supported (the shipped value, putslammatcherOpenCVParameters.xml:37) */
    int32_t iterationCount;   /* ignored on input, like the reference ctor (RANSAC.cpp:30) */
} PsRansacParams;

/* Which sequential selection rule is replayed over the per-hypothesis inlier counts. */
typedef enum PsEstimator {
    PS_EST_RANSAC = 0,  /* RANSAC.cpp:87-164: strict-> best ratio, adaptive iterationCount, refit, ratio gate */
    PS_EST_USAC = 1,    /* USAC.h:326,409-414,944-971 + USAC_wrapper.cpp:104-151: best count, std stopping, no refit */
    PS_EST_FIXED = 2    /* all H hypotheses, first best wins, then RANSAC's refit + gate (adaptive stop disabled) */
} PsEstimator;

/* Controls that have no counterpart in the reference because its sampling is
 * srand(time(0)) + rand() (RANSAC.cpp:13,191): the sample stream is an input. */
typedef struct PsRansacConfig {
    int32_t estimator;        /* PsEstimator */
    int32_t numHypotheses;    /* H: number of 3-point samples that may be consumed (>= the schedule's maximum) */
    uint64_t seed;            /* counter-based stream: draw(h,j) = mix(seed,h,j) >> 33, index = draw % M, redraw on repeat */
    const uint32_t *sampleIdx;/* optional HOST pointer, H x 3 raw draws replacing the seeded stream:
                                 index_j = raw % M, a repeat is moved to the next free index (+1 mod M) */
} PsRansacConfig;

typedef struct PsRansacStats {
    int32_t numMatchesIn;     /* matches handed in (cross-check survivors) */
    int32_t numMatchesValid;  /* M after the depth filter RANSAC.cpp:65-74 */
    int32_t bestHypothesis;   /* index of the selected sample, -1 if none */
    int32_t bestInlierCount;  /* its inlier count inside the loop */
    int32_t iterationsRun;    /* loop trips the sequential reference would have made */
    int32_t numInliers;       /* final inliers (after refit re-selection and the ratio gate) */
    int32_t accepted;         /* 0 => identity returned (too few matches or ratio gate) */
    float bestInlierRatio;    /* float(count)/float(M) as in RANSAC.cpp:280 */
    double pointInlierRatio;  /* RANSAC::pointInlierRatio, RANSAC.h:56-66 (NaN if no input matches) */
} PsRansacStats;

typedef struct PsContext PsContext;

/* ---- context: one HIP stream + scratch arena per instance (reference threading
 * contract: main-thread matcher and loop-closure matcher are separate instances,
 * PUTSLAM.cpp:566,570; featuresMap.cpp:650-652,794). ------------------------- */
int ps_context_create(int device, PsContext **out);
void ps_context_destroy(PsContext *ctx);
/* Use an externally owned hipStream_t (e.g. the caller's current stream); NULL restores the private stream, which
 * is created hipStreamNonBlocking: it is NOT ordered with the legacy default stream, so a caller working on the
 * default stream hands over an explicit stream (forked from / joined to the default one) or synchronises.
 * The scratch arena belongs to the context: when the stream changes, the new stream is made to wait for the event
 * recorded at the end of the last asynchronous call (ps_vo_pairs_device), so consecutive calls on different streams
 * never overlap on it.  The previous stream itself is not touched by ps_context_set_stream: its owner may destroy it once
 * the calls submitted to it have been synchronised or a later stream has been selected.
 * One context still serves one caller thread at a time; concurrent chains use one context each. */
int ps_context_set_stream(PsContext *ctx, void *hipStream);
int ps_context_synchronize(PsContext *ctx);
/* The hipStream_t the context's calls are queued on (its private stream unless ps_context_set_stream chose another) and the
 * device it was created for: what a host needs to order its own kernels, copies or collectives with the context's work
 * (include/putslam_shard.h queues its RCCL calls there). */
void *ps_context_stream(PsContext *ctx);
int ps_context_device(const PsContext *ctx);
/* Kernel variants kept side by side for A/B measurements and as tested twins (results are identical):
 *   "matcher": 1 = FP4 matrix-core sweep ps_hamming_mfma, 0 = integer VALU sweep ps_hamming_nn, 2 = by batch size
 *              (default: the matrix-core form, one launch more, from about five 2000-keypoint pairs per call on)
 *              (environment: PUTSLAM_HIP_MATCHER=mfma|valu|auto, read at context creation); "matcher_used" (read only)
 *              tells which of the two the last matching call ran.
 *   "score":   1 = decision-exact fast scoring kernels (cheap evaluation with a proven error band, in-band evaluations
 *              re-done by the value-exact code; default): ps_ransac_score_euclid for errorVersion 0 / 4 (the metric every
 *              shipped reference config runs), ps_ransac_score_fast for errorVersion 1 / 2;
 *              0 = value-exact ps_ransac_score<M> for every evaluation (PUTSLAM_HIP_SCORE=fast|exact).
 *              Per-hypothesis counts are identical between 0 and 1 by proof + tests.  (Round 2's matrix-core experiment,
 *              value 2, left the library in round 4: profiles/variants/ps_score_mfma.h.txt.)
 *   "prune":   1 (default) = staged scoring of large batches: the first 256 hypotheses of every pair are scored
 *              completely, the later ones in three stages over growing match ranges; between the stages every
 *              hypothesis that cannot become a record of the sequential selection any more (count so far + matches left
 *              <= best count of the earlier ones, RANSAC.cpp:438-455) is abandoned, and hypotheses beyond the adaptive
 *              trip limit (RANSAC.cpp:450-453) are never started; all outputs are unchanged, only the scratch counts of
 *              abandoned hypotheses are lower bounds.  "Large" is decided by a cost model: pairs x (ceil(H / 256) - 1) x
 *              maxKpts against base + perRow x maxKpts, per metric family and schedule (the staged form costs six or seven
 *              dependent launches and pays them back with the evaluations it abandons).  2 = the staged form whenever the
 *              kernels have it (H > 256), whatever the batch size; 0 = every hypothesis is scored completely
 *              (PUTSLAM_HIP_PRUNE=0|1|2).  The diagnostic ps_debug_ransac_counts always scores completely.
 *   "reorder": the stages after the first sweep a copy of the pair's match record in which the matches the best hypotheses
 *              so far reject come first (written by a launch of its own between the stages): whatever is not better than
 *              those hypotheses rejects nearly all of them too and is abandoned a few matches later.  Counts are sums over
 *              all matches, so the order changes no output.  1 = always, 0 = original match order, 2 (default) = with the
 *              fixed schedule only (under the adaptive ones the trip limit usually ends the scoring before the stages
 *              start and the launch would buy nothing)  (PUTSLAM_HIP_REORDER=0|1|2).
 *   "bail":    1 (default) = "nothing to gain" handling of the staged scoring for the Euclidean metrics: a pair whose prefix
 *              leaves a miss budget so large that the first stage sweeps every match anyway skips the reorder vote, and -- fixed
 *              schedule only -- while most pairs of the last observed batched call OF THE SAME KIND (metric, schedule, H,
 *              batch-size class, frame capacity, frame set; eight kinds are tracked) were such pairs, the next calls of that
 *              kind are scored completely, probing with the staged form every 16th call (identical outputs either way;
 *              "hopeless", read only, is the state of the last call's kind).  Adaptive schedules always keep the staged form.
 *              0 = always the staged form.  Setting the option (to either value) forgets what was observed.
 *   "last_staged_pairs" / "last_reordered_pairs" (read only): pairs of the last scoring step if it was staged / reordered,
 *              else 0.
 *   "model_room_mib": room for the staged scoring's parked models (48 bytes per pair and leading hypothesis); 0 (default) =
 *              256 MiB under the adaptive schedules, 2 GiB under the fixed one.  Hypotheses without a slot are swept in one
 *              piece by stage 1 and rebuilt by kernel 4 if one of them wins: identical outputs, tests force it small.
 *   "score_stats": 1 = count the evaluations the fast kernel hands to the value-exact code (ps_debug_score_stats).
 *   "stamps":  1 = kernels 2 and 4 record the shader clock at their phase boundaries (ps_debug_stamps); 0 (default) = they
 *              are passed a null pointer and record nothing.
 *   "side_by_side": 0 (default) = the context's launches have the chip to themselves; n >= 2 = it is one of n launch chains
 *              that run side by side (a PsBatchQueue sets it on its chains, the pipelined stream on its lanes from chunks of 48
 *              frames on; a host that drives several contexts on streams of its own sets it itself).  The other chains fill the
 *              gaps between the staged scoring's dependent launches, so "prune" = 1 takes the staged form from far smaller
 *              batches on (E1 / fixed / H = 4096 / 2000 keypoints: from 16 pairs instead of 77; two chains: from 35).  Identical
 *              outputs whatever the value  (PUTSLAM_HIP_SIDE_BY_SIDE).
 * Twelve options in all are the surface: "matcher", "matcher_fused", "score", "prune", "side_by_side", "reorder", "bail", "model_room_mib",
 * "stream_copy_kernels", "stream_ahead" (places of the pipelined stream beyond one per lane, see below), "score_stats", "stamps",
 * and the read-only ones.
 * NOT part of it -- launch-shape and tuning knobs of the sweeps and of the staged scoring, every value of which gives the same
 * results; they exist for the parity tests (tests/test_gpu_prune.py runs every one next to the default) and for A/B
 * measurements, answer only to the name "debug.<knob>" (and PUTSLAM_HIP_<KNOB> at context creation) and may change between
 * versions: qsplit / msplit (work-groups the query range of kernel 1 / the match range of kernel 3 is split over, 0 =
 * automatic), gensplit (stage 0 as two launches, models then sweep), singlerest (one stage after the prefix under the adaptive
 * schedules), pretest (stage 1's one-direction pre-test), prefix (64 / 128 / 192 / 256 hypotheses of stage 0), list_g2
 * (work-groups per pair of stage 2), reorder_top (voters), reorder_margin.  (list_g3, list_r3, reorder_c2div and reorder_gran
 * left in round 6: every A/B had their other values within 1 % of the defaults; they are constants of the library now.)
 * ps_context_get_option returns the value or a negative PsStatus. */
int ps_context_set_option(PsContext *ctx, const char *name, int value);
int ps_context_get_option(const PsContext *ctx, const char *name);
const char *ps_last_error(const PsContext *ctx);
int ps_abi_version(void);
/* Name of the device the context runs on, e.g. "gfx950". */
const char *ps_device_arch(const PsContext *ctx);

/* ---- A1: MatcherOpenCV::performMatching, src/Matcher/matcherOpenCV.cpp:198-206
 * = cv::BFMatcher(NORM_HAMMING, crossCheck=true).match(query=prev, train=cur)
 * (matcher object built at matcherOpenCV.cpp:100-105).  Host pointers; rows are
 * 32 bytes wide with a row pitch of qstep/tstep bytes (cv::Mat::step).
 * out must hold nq entries; *nout receives the number written (ascending queryIdx). */
int ps_match_hamming256(PsContext *ctx,
                        const uint8_t *query, int nq, size_t qstep,
                        const uint8_t *train, int nt, size_t tstep,
                        PsDMatch *out, int *nout);

/* ---- A4-A9 / A11: RANSAC::estimateTransformation, src/TransformEst/RANSAC.cpp:50-174
 * and RANSAC_USAC::estimateTransformation, src/USAC/USAC_wrapper.cpp:104-151.
 * prev/cur: N x 3 floats, 12-byte stride (std::vector<Eigen::Vector3f> storage).
 * K: row-major 3x3 float camera matrix (cv::Mat CV_32FC1, RGBD.cpp:93-96); may be NULL for
 *    the Euclidean/adaptive modes.
 * pose: column-major 4x4 float (Eigen::Matrix4f storage), maps current-frame points into
 *    the previous frame (umeyama(src=cur,dst=prev), RANSAC.cpp:225-226).
 * inliers (capacity m) / ninl: final inlier matches in input order; mask (m bytes, may be
 *    NULL): 1 where matches[i] is a final inlier. stats may be NULL. */
int ps_ransac_rigid3d(PsContext *ctx, const PsRansacParams *params, const PsRansacConfig *cfg,
                      const float *K,
                      const float *prev, int nprev, const float *cur, int ncur,
                      const PsDMatch *matches, int m,
                      float *pose, PsDMatch *inliers, int *ninl, uint8_t *mask,
                      PsRansacStats *stats);

/* ---- A7: RANSAC::computeTransformationModel, RANSAC.cpp:207-244
 * (Eigen::umeyama(src, dst, false) in float + the isnan(T(0,0)) check).
 * nsets independent fits of k points each: src/dst are nsets x k x 3 floats.
 * T: nsets x 16 column-major; valid: nsets flags (0 => identity written). */
int ps_umeyama_f32(PsContext *ctx, const float *src, const float *dst, int k, int nsets,
                   float *T, int32_t *valid);

/* ---- A10: KabschEst::computeTransformation, src/TransformEst/kabschEst.cpp:24-68
 * (interface include/putslam/TransformEst/transformEst.h:23).
 * A, B: n x 3 doubles, COLUMN-major with leading dimension ld (Eigen::MatrixXd storage).
 * T: column-major 4x4 double (Mat34 = Eigen::Transform<double,3,Affine>), maps A onto B.
 * Only rows 0 .. n-1 of each column are read (ld > n: the rows between are padding).  The rotation is proper for every
 * input: its handedness comes from the SVD's factors (det V det W), where kabschEst.cpp:53 takes the sign of the
 * covariance's determinant -- the same for a covariance of full rank, rounding noise (a reflection for every second
 * planar, collinear or three-point set) otherwise.  The summation order is a function of n alone: the same bytes for the
 * same input, whatever ran before. */
int ps_kabsch_f64(PsContext *ctx, const double *A, const double *B, int n, int ld, double *T);

/* ---- A3: RGBD::keypoints2Dto3D / point2Dto3D / roundSize, src/RGBD/RGBD.cpp:10-16,30-65.
 * xy: n x 2 floats (cv::Point2f), depth: rows x cols uint16 with a pitch of depthStep BYTES,
 * K row-major 3x3 float, out: n x 3 floats.
 * depth may be a region of a larger image (cv::Mat ROI, depthStep > cols * 2): the call reads
 * ps_depth_view_bytes(rows, cols, depthStep) bytes from `depth` and no more.  A rounded pixel (v, u) is read by the
 * reference's pointer arithmetic, so u == cols in a row that is not the last yields what follows that row's pixels (the
 * parent image's next pixel; the next row's first pixel when dense); an address at or past the end of the last row's
 * pixels (u == cols there, v == rows) yields depth 0 = missing, where the reference reads out of bounds.
 * A NaN x or y has no pixel (the reference's (int)round(NaN) is undefined): depth 0 = missing, so Z = 0 (for a
 * depthImageScale that is not 0) and X, Y are what (x - cx) / fx * Z gives: NaN for the NaN coordinate. */
int ps_keypoints2Dto3D(PsContext *ctx, const float *xy, int n,
                       const uint16_t *depth, int rows, int cols, size_t depthStep,
                       const float *K, double depthImageScale, float *out);

/* The addressable bytes of a rows x cols uint16 image with a pitch of depthStep bytes:
 * (rows - 1) * depthStep + cols * 2 (the last row ends after its pixels, not after a whole pitch).
 * 0 for a shape ps_keypoints2Dto3D rejects (rows or cols < 1, depthStep < cols * 2).  Needs no context and no device. */
size_t ps_depth_view_bytes(int rows, int cols, size_t depthStep);

/* ---- N4: RGBD::removeImageDistortion, src/RGBD/RGBD.cpp:254-314 = cv::undistortPoints(pts, K, dist) with
 * R = P = I (5 fixed-point iterations of the Brown model, double) followed by u = x_n*fx + cx in float.
 * xy, out: n x 2 floats (cv::Point2f); dist5 = (k1, k2, p1, p2, k3) (datasetConfig rgbDistortion). */
int ps_remove_image_distortion(PsContext *ctx, const float *xy, int n, const float *K, const double *dist5,
                               float *out);

/* ---- A3: RGBD::point3Dto2D, src/RGBD/RGBD.cpp:92-98 (n points). */
int ps_points3Dto2D(PsContext *ctx, const float *xyz, int n, const float *K, float *uv);

/* ---- DBScan keypoint thinning: DBScan(eps, minPts, featuresFromCluster).run(keypoints), src/Matcher/dbscan.cpp
 * (include/putslam/Matcher/dbscan.h; run between detection and description, matcher.cpp:24-26,221-223,459-461,561-563).
 * Two keypoints are neighbours iff (float)cv::norm(pt_i - pt_j) < eps; a cluster keeps its first featuresFromCluster
 * members in index order (none if that is <= 0), noise is kept, and a keypoint whose octave already is -5 (the reference's
 * erase marker) is removed.  keptIdx (room for n entries: the call may write all n) receives the survivors' indices in
 * ascending order, *nkept their number.
 * xy: n points of two floats, xyStride BYTES apart (0 = 8: packed cv::Point2f; sizeof(cv::KeyPoint) with &kps[0].pt);
 * octave: n int32, octaveStride BYTES apart (0 = 4), or NULL (no -5 rule).  Host pointers; synchronous on the context's
 * stream.  n <= PS_DBSCAN_MAX_KPTS (per-point state lives in LDS). */
#define PS_DBSCAN_MAX_KPTS 8000
int ps_dbscan_thin(PsContext *ctx, const float *xy, size_t xyStride, const int32_t *octave, size_t octaveStride, int n,
                   double eps, int minPts, int featuresFromCluster, int32_t *keptIdx, int *nkept);
/* The same over a DEVICE-resident batch, one work-group per frame: xy frames x capacity x 2 floats, octave frames x capacity
 * int32 (or NULL), counts frames int32 (points of each frame, 0 .. capacity); keptIdx frames x capacity int32 (frame f's
 * survivors at f x capacity, ascending), nkept frames int32 (-1 for a frame whose count lies outside 0 .. capacity).
 * capacity <= PS_DBSCAN_MAX_KPTS.  Asynchronous on the context's stream; uses no scratch of the context. */
int ps_dbscan_thin_device(PsContext *ctx, const float *xy, const int32_t *octave, const int32_t *counts, int frames,
                          int capacity, double eps, int minPts, int featuresFromCluster, int32_t *keptIdx, int32_t *nkept);

/* ---- Spatial-exclusion filters: candidates that lie too close to features already held are rejected.  One rule type covers
 * the three loops of the reference's front end; every predicate is decided as  squared sum < bound  with the bound found on
 * the host (no device sqrt), and is false when a NaN is involved.
 *   form3 = PS_EXCL_F32: float differences, float sum d0*d0 + (d1*d1 + d2*d2), (double)sum < bound3 -- Eigen's
 *           (a - b).norm() < d on Vector3f with bound3 = ps_map_sphere_bound(d) (PUTSLAM.cpp:58-62,81-85);
 *   form3 = PS_EXCL_F64: the doubles of the float differences, x*x + y*y + z*z summed left to right, sum < bound3
 *           (matcher.cpp:905-908 with bound3 = ps_sqrt_bound_f64(d));
 *   form2 = PS_EXCL_F64: (double)du*du + (double)dv*dv < bound2 with float du, dv -- cv::norm(p - q) < d with
 *           bound2 = ps_sqrt_bound_f64(d) (matcher.cpp:114-116,910-912), (float)cv::norm(p - q) < d with
 *           bound2 = ps_debug_dbscan_bound(d) (PUTSLAM.cpp:66-68,89-91);
 *   PS_EXCL_NONE: that test is absent.  Two points are near iff either test passes.
 *   mode PS_EXCL_GREEDY: candidates are walked in ascending index; one is accepted iff it passes the depth gate, no
 *           existing feature is near it and no candidate accepted before is near it.
 *   mode PS_EXCL_ALL_EARLIER: a candidate is kept iff it passes the depth gate, no existing feature is near it and NO
 *           earlier candidate is near it, kept or not.
 *   depthGate != 0: only candidates with (double)z > depthMin && (double)z < depthMax pass (PUTSLAM.cpp:117).
 *   maxKeep >= 0: the result is cut after its first maxKeep members (PUTSLAM.cpp:113); < 0: no cap. */
enum { PS_EXCL_NONE = 0, PS_EXCL_F32 = 1, PS_EXCL_F64 = 2 };
enum { PS_EXCL_GREEDY = 0, PS_EXCL_ALL_EARLIER = 1 };
typedef struct PsExclusionRule {
    double bound3;
    double bound2;
    double depthMin, depthMax;
    int32_t form3;     /* PS_EXCL_NONE / PS_EXCL_F32 / PS_EXCL_F64 */
    int32_t form2;     /* PS_EXCL_NONE / PS_EXCL_F64 */
    int32_t mode;      /* PS_EXCL_GREEDY / PS_EXCL_ALL_EARLIER */
    int32_t maxKeep;
    int32_t depthGate;
    int32_t reserved;  /* 0 */
} PsExclusionRule;
size_t ps_abi_sizeof_exclusion_rule(void);

/* The least double s with sqrt(s) >= d (the correctly rounded double root): sqrt(t) < d  <=>  t < s for every t >= 0.
 * 0 for d <= 0 or NaN (nothing passes), +inf for d = +inf.  Pure host arithmetic. */
double ps_sqrt_bound_f64(double d);

/* Rule constructors, pure host arithmetic (no context, no device); PS_ERR_BAD_ARG for a NULL rule.
 * new_map_features: PUTSLAM::chooseFeaturesToAddToMap + removeCloseFeatures, src/PUTSLAM/PUTSLAM.cpp:53-178 -- greedy, 3-D float
 *   norm or 2-D float-rounded norm, depth gate (0.8, 6.0), cap maxOnceFeatureAdd (<= 0: nothing is accepted).  Both thresholds
 *   pass through a float parameter there (:101) and are rounded to float here.  A caller that continues a count passes
 *   maxOnceFeatureAdd - addedCounter.
 * merge_tracked: Matcher::mergeTrackedFeatures, src/Matcher/matcher.cpp:97-130 -- greedy, 2-D double norm, no gate, no cap.
 * too_close: Matcher::removeTooCloseFeatures, matcher.cpp:886-974 -- all-earlier, 3-D and 2-D double norms. */
int ps_exclusion_rule_new_map_features(double minEuclideanDistanceOfFeatures, double minImageDistanceOfFeatures,
                                       int maxOnceFeatureAdd, PsExclusionRule *rule);
int ps_exclusion_rule_merge_tracked(double minimalReprojDistanceNewTrackingFeatures, PsExclusionRule *rule);
int ps_exclusion_rule_too_close(double minimalEuclidDistanceNewTrackingFeatures, double minimalReprojDistanceNewTrackingFeatures,
                                PsExclusionRule *rule);

/* The filter.  cand3: n x 3 floats (feature3D), cand2: n x 2 floats (undistortedFeature2D); exist3 / exist2: the m features
 * already held, the float casts of their position and (u, v) made by the caller (as with mapPos of ps_match_xyz).  A 3-D array
 * may be NULL when the rule has neither a 3-D test nor a depth gate, a 2-D array when it has no 2-D test; the existing arrays
 * also when m = 0.  keptIdx (room for n entries) receives the indices of the accepted candidates, ascending, *nkept their
 * number.  Host pointers; synchronous on the context's stream.
 * n <= PS_EXCL_MAX_CAND (per-candidate state lives in LDS), m <= PS_MAX_KPTS, else PS_ERR_UNSUPPORTED; a NULL where an array is
 * needed, a negative count or a rule with an unknown form or mode -> PS_ERR_BAD_ARG (text: ps_last_error).  Outputs are not
 * touched on an error. */
#define PS_EXCL_MAX_CAND 8192
int ps_exclude(PsContext *ctx, const PsExclusionRule *rule, const float *cand3, const float *cand2, int n, const float *exist3,
               const float *exist2, int m, int32_t *keptIdx, int *nkept);
/* The same over a DEVICE-resident batch of frames: cand3 frames x candCapacity x 3, cand2 frames x candCapacity x 2, candCounts
 * frames int32; exist3 / exist2 / existCounts likewise with existCapacity (0: no existing set, the three may be NULL).
 * keptIdx frames x candCapacity int32 (frame f's survivors at f x candCapacity), nkept frames int32: -1 for a frame one of whose
 * counts lies outside 0 .. its capacity.  Asynchronous on the context's stream, copies nothing; the context's scratch holds
 * 5 bytes per frame and candidate slot. */
int ps_exclude_device(PsContext *ctx, const PsExclusionRule *rule, const float *cand3, const float *cand2,
                      const int32_t *candCounts, int candCapacity, const float *exist3, const float *exist2,
                      const int32_t *existCounts, int existCapacity, int frames, int32_t *keptIdx, int32_t *nkept);

/* ---- N2: guided map matching, core of Matcher::matchXYZ, src/Matcher/matcher.cpp:606-746.
 * For every map feature j: candidates i among the current frame's keypoints with
 * |mapPos[j] - curPos[i]| < sphereRadius and |curLevel[i] - mapLevel[j]| <= 1 (:699-711); their value is
 * cv::norm(mapDesc[j] - curDesc[i], NORM_HAMMING) on CV_8U rows = popcount of the per-byte SATURATING
 * difference (:719-721); every candidate with acceptRatio * value <= best value is emitted (:734-746) as
 * DMatch(queryIdx = j, trainIdx = i, imgIdx = -1, distance = value), ordered by (j, i).
 * mapPos: (float) casts of MapFeature::position (:701-702); levels from ps_predicted_level.
 * Returns PS_ERR_BAD_ARG with *nout = required capacity if cap is too small; out is then not written.  Host pointers,
 * synchronous.  A row pitch below 32 bytes or more than PS_MAX_KPTS rows on either side -> PS_ERR_UNSUPPORTED; NULL where an
 * array is needed -> PS_ERR_BAD_ARG; *nout = 0 on those errors.  An empty side gives no matches (PS_OK). */
int ps_match_xyz(PsContext *ctx, const float *mapPos, const uint8_t *mapDesc, size_t mapDescStep,
                 const int32_t *mapLevel, int nmap, const float *curPos, const uint8_t *curDesc,
                 size_t curDescStep, const int32_t *curLevel, int ncur, double sphereRadius,
                 double acceptRatio, PsDMatch *out, int cap, int *nout);
/* Predicted ORB pyramid level, matcher.cpp:639-652 (keypoints) and :681-692 (map features):
 * clamp(ceil(log(1.2^octave * detDist / curDist) / log 1.2), 0, 7).  Pure host arithmetic (libm). */
int ps_predicted_level(int octave, double detDist, double curDist);

/* ---- A2 + A12: the data flow of Matcher::match (src/Matcher/matcher.cpp:470-515) for a
 * whole batch of independent frame pairs, everything resident in HBM.  All pointers in
 * PsFrameSet / PsPairResults are DEVICE pointers; nothing is copied to or from the host. */
typedef struct PsFrameSet {
    const uint8_t *desc;      /* numFrames x maxKpts x 32 B descriptors */
    const float *pts;         /* numFrames x maxKpts x 3 floats, back-projected 3-D points */
    const int32_t *nkpts;     /* numFrames keypoint counts (<= maxKpts) */
    int32_t numFrames;
    int32_t maxKpts;          /* row capacity per frame; also the capacity of per-pair outputs */
    /* ABI 2: bytes from one frame's block to the next; 0 = dense (maxKpts x 32 / maxKpts x 12).  A frame set whose frames keep
     * their descriptors and points together -- [maxKpts x 32 B][maxKpts x 12 B] per frame, what one transfer per frame or per
     * chunk of frames delivers (the prevDescriptors / prevFeatures3D pair of matcher.h:379-384 as one block) -- has
     * pts = desc + maxKpts x 32 and both strides = the frame's size.  descFrameStride: a multiple of 16, >= maxKpts x 32;
     * ptsFrameStride: a multiple of 4, >= maxKpts x 12; desc itself 16-byte aligned.  Every call that takes a frame set applies
     * this one rule, and refuses a stride whose quarter does not fit an int (8 GiB and more between frames) with PS_ERR_BAD_ARG. */
    size_t descFrameStride;
    size_t ptsFrameStride;
} PsFrameSet;

typedef struct PsPairResults {
    PsDMatch *matches;        /* P x maxKpts: cross-check matches per pair, ascending queryIdx */
    int32_t *numMatches;      /* P */
    uint8_t *inlierMask;      /* P x maxKpts: 1 where matches[p][i] is a final inlier */
    float *pose;              /* P x 16 column-major */
    PsRansacStats *stats;     /* P */
} PsPairResults;

/* pairs: DEVICE array of P (prevFrame, curFrame) index pairs, int32 x 2 each.
 * Hypothesis h of pair p draws from the seeded stream with seed cfg->seed + p
 * (cfg->sampleIdx must be NULL). Asynchronous on the context's stream.
 * Scratch: counts take 4 bytes per pair and hypothesis of cfg->numHypotheses (1.7 GB for 499 pairs under USAC's cap of
 * 850 000, USAC_wrapper.cpp:70; touched only up to each pair's trip limit); the staged scoring's parked models take 48 bytes
 * per pair and LEADING hypothesis, 256 MB at most under the adaptive schedules (2 GiB under the fixed one): a hypothesis
 * beyond the slots is swept in one piece and, should it win, rebuilt (options "arena_mib", "last_model_slots", read only).
 * Throughput: a host that loops over batches gets 18 % more (499 pairs) to 2.9 x (64 pairs) from a PsBatchQueue (below), which
 * hands the batches to four contexts on four streams in turn -- launch chains that are never joined. */
int ps_vo_pairs_device(PsContext *ctx, const PsRansacParams *params, const PsRansacConfig *cfg,
                       const float *K, const PsFrameSet *frames,
                       const int32_t *pairs, int P, const PsPairResults *out);

/* ---- A1 for FLOAT descriptors (SURF / SIFT): MatcherOpenCV::performMatching, src/Matcher/matcherOpenCV.cpp:198-206, with the
 * matcher the plugin builds for those two settings, cv::BFMatcher(cv::NORM_L2, crossCheck = true) (matcherOpenCV.cpp:100-102).
 * The semantics are RESTATED, not compiled against an OpenCV:
 *   L2sqr(a, b) in float, every operation rounded separately, no FMA, in the order of OpenCV 3.0 - 3.3's SSE2 normL2Sqr_: eight
 *     lane accumulators over the blocks of eight elements, d = ((s0 + s1) + s2) + s3 over s[i] = acc0[i] + acc1[i], then
 *     d += ((t0^2 + t1^2) + t2^2) + t3^2 over blocks of four differences, then d += t^2 per element;
 *   dist = sqrtf(L2sqr), correctly rounded; every comparison is made on dist (two different sums may share a square root);
 *   step 1: each train row takes the query row with the least dist < FLT_MAX, ties to the lowest index (NaN, +inf and values
 *     >= FLT_MAX are never taken; a train row without an admissible query takes nobody);
 *   step 2: each query row keeps the train row with the least dist among those that took it, ties to the lowest index;
 *   step 3: DMatch(q, t, 0, dist) in ascending q.
 * Every distance is computed value-exactly by HIP kernels (no CPU path): outputs are byte for byte the restatement's.
 * Host pointers, synchronous; rows are dim floats wide, 1 <= dim <= PS_MAX_L2_DIM, with a row pitch of qstep / tstep BYTES
 * (cv::Mat::step, >= dim x 4).  out must hold nq entries; *nout receives the number written.
 * Option "matcher_l2" (environment PUTSLAM_HIP_MATCHER_L2, read at context creation): 1 (default) = for dim 64 / 128 a
 * matrix-core prefilter (v_mfma_f32_32x32x2_f32) lists, per train row, the queries a proven error band cannot exclude, and only
 * those are evaluated value-exactly; 0 = every (t, q) is.  The bytes are the same; "matcher_l2_used" (read only) reports the form
 * the last call took.
 * dim < 1, a pitch below a row, NULL where an array is needed -> PS_ERR_BAD_ARG; dim > PS_MAX_L2_DIM or more than PS_MAX_KPTS
 * rows -> PS_ERR_UNSUPPORTED; *nout = 0 on error. */
#define PS_MAX_L2_DIM 512
int ps_match_l2_f32(PsContext *ctx, const float *query, int nq, size_t qstepBytes, const float *train, int nt, size_t tstepBytes,
                    int dim, PsDMatch *out, int *nout);

/* A frame set with float descriptors; all pointers are DEVICE pointers.  THE RULES: desc is 4-byte aligned; descRowStride is a
 * multiple of 4 and >= dim x 4 (0 = dense, dim x 4); descFrameStride is a multiple of 4 and >= maxKpts x the row stride (0 =
 * dense); ptsFrameStride is a multiple of 4 and >= maxKpts x 12 (0 = dense), its quarter fits an int.  What lies between the
 * rows is never read. */
typedef struct PsFrameSetF32 {
    const float *desc;        /* numFrames x maxKpts rows of dim floats */
    const float *pts;         /* numFrames x maxKpts x 3 floats, back-projected 3-D points (may be NULL for ps_match_l2_device) */
    const int32_t *nkpts;     /* numFrames keypoint counts (<= maxKpts) */
    int32_t numFrames;
    int32_t maxKpts;          /* row capacity per frame; also the capacity of per-pair outputs */
    int32_t dim;              /* floats per descriptor: 64 (SURF), 128 (SIFT / extended SURF), any 1 .. PS_MAX_L2_DIM */
    size_t descRowStride;     /* bytes between rows, 0 = dense */
    size_t descFrameStride;   /* bytes between frames' descriptor blocks, 0 = dense */
    size_t ptsFrameStride;    /* bytes between frames' point blocks, 0 = dense */
} PsFrameSetF32;
size_t ps_abi_sizeof_frameset_f32(void);

/* matcherOpenCV.cpp:100-102,198-206 for P (prevFrame, curFrame) pairs of a device-resident set: matches (P x maxKpts) and
 * numMatches (P) are DEVICE arrays; asynchronous on the context's stream, nothing is copied to or from the host.  Pair p's list
 * is byte for byte ps_match_l2_f32's on the two frames.  A pair that names a frame outside the set has no matches.
 * NULL where an array is needed, P < 0, dim < 1, a bad stride -> PS_ERR_BAD_ARG; dim > PS_MAX_L2_DIM or maxKpts > PS_MAX_KPTS ->
 * PS_ERR_UNSUPPORTED; the outputs are not touched.  P == 0 is PS_OK. */
int ps_match_l2_device(PsContext *ctx, const PsFrameSetF32 *frames, const int32_t *pairs, int P, PsDMatch *matches,
                       int32_t *numMatches);

/* The body of ps_vo_pairs_device with the float matcher (matcherOpenCV.cpp:100-102,198-206) in front: pair p draws from
 * cfg->seed + p, and every output is byte for byte what ps_match_l2_f32 followed by ps_ransac_rigid3d with seed + p gives.
 * Argument rules as ps_match_l2_device (frames->pts is needed here). */
int ps_vo_pairs_l2_device(PsContext *ctx, const PsRansacParams *params, const PsRansacConfig *cfg, const float *K,
                          const PsFrameSetF32 *frames, const int32_t *pairs, int P, const PsPairResults *out);

/* ---- N2 for a device-resident batch: Matcher::matchXYZ (src/Matcher/matcher.cpp:606-798) for P (map view, frame) pairs --
 * guided matching, then the estimator -- as ONE launch chain.  PUTSLAM calls matchXYZ once per frame and retries it up to ten
 * times with a wider sphere and a looser ratio while the inlier ratio stays under 0.1 (src/PUTSLAM/PUTSLAM.cpp:788-798): the
 * tries of one frame, or the frames of many sequences, are one batch here.
 * ps_map_sphere_bound: the least float B with  (float)|a - b| < sphereRadius  <=>  squared sum < B  (what ps_match_xyz computes
 * internally); 0 for a radius that is 0, negative or NaN (nothing passes), +inf beyond sqrt(FLT_MAX).  Pure host arithmetic,
 * so a caller can fill a per-pair array. */
float ps_map_sphere_bound(double sphereRadius);

typedef struct PsMapBatch {
    PsFrameSet maps;              /* "map views": per view the visible map features -- desc = the descriptor chosen for
                                     each (matcher.cpp:675-679), pts = (float) casts of MapFeature::position in the
                                     camera frame (:700-701), nkpts = features per view.  Strides as in ABI 2. */
    const int32_t *mapLevel;      /* maps.numFrames x maps.maxKpts predicted levels (ps_predicted_level, :681-692) */
    PsFrameSet frames;            /* current frames: descriptors + back-projected points */
    const int32_t *curLevel;      /* frames.numFrames x frames.maxKpts (:639-652) */
    const int32_t *pairs;         /* P x 2 (map view, frame), device */
    int32_t P;
    int32_t maxMatches;           /* row capacity of out->matches / out->inlierMask for every pair */
    float radiusBound;            /* ps_map_sphere_bound(radius), used when radiusBoundPerPair is NULL */
    double acceptRatio;           /* used when acceptRatioPerPair is NULL */
    const float *radiusBoundPerPair;   /* device, P, or NULL */
    const double *acceptRatioPerPair;  /* device, P, or NULL */
} PsMapBatch;

/* All pointers inside PsMapBatch and PsPairResults are DEVICE pointers.  Both calls are asynchronous on the context's stream,
 * copy nothing to or from the host and do not synchronise (growing the context's scratch on a first call aside, as with
 * ps_vo_pairs_device).
 *   matches: P x maxMatches; pair p's list is exactly what ps_match_xyz returns for that map view and frame with that pair's
 *     radius and ratio: candidates by sphere and |level difference| <= 1 (:699-711), value = popcount of the per-byte
 *     SATURATING difference mapDesc - curDesc (:719-721), best = smallest value with the first index on ties (:714-727), every
 *     candidate with acceptRatio * value <= best emitted as DMatch(j, i, -1, value) (:734-746), ordered by (j, i).
 *   numMatches[p]: the count.  If it exceeds maxMatches, numMatches[p] = -(count), nothing of that pair's rows need be
 *     meaningful and the estimator treats the pair as having no matches; other pairs are unaffected (ps_match_xyz's "returns
 *     the needed capacity" rule, per pair and without a round trip).  A pair that names a view or a frame outside its set has
 *     no matches.
 * ps_map_pairs_device then runs the estimator of cfg with params->errorVersion as given (the caller sets errorVersionMap, as
 * with ps_ransac_rigid3d) on prev = maps.pts, cur = frames.pts; pair p draws from cfg->seed + p; cfg->sampleIdx must be NULL.
 * Mask, pose and every field of PsRansacStats are byte for byte those of ps_match_xyz followed by ps_ransac_rigid3d with
 * seed + p on the same pair.  A pair without matches gives identity, numInliers = 0, accepted = 0, pointInlierRatio = NaN
 * (the wrappers turn that into the reference's -1.0, matcher.cpp:755-756); an overflowed pair's stats.numMatchesIn is 0.
 * Limits: maxKpts of either set above PS_MAX_KPTS or maxMatches above 1 << 22 -> PS_ERR_UNSUPPORTED; maxMatches < 1, bad
 * strides (the rule of PsFrameSet), NULL where an array is needed, P < 0 -> PS_ERR_BAD_ARG (text: ps_last_error); outputs are
 * not touched.  P == 0 is PS_OK.
 * Scratch grows with P x maxMatches: 16 B a match for the staging rows and, for ps_map_pairs_device, about 150 B a match for
 * the scoring records (0.6 GB for 499 pairs x 8000); size maxMatches to the tries that are run (4 x maxKpts holds the tenth
 * try of the retry ladder on the test scenes, maxKpts the first).  The keys block the VO calls share is not touched. */
int ps_match_xyz_device(PsContext *ctx, const PsMapBatch *b, PsDMatch *matches, int32_t *numMatches);
int ps_map_pairs_device(PsContext *ctx, const PsRansacParams *params, const PsRansacConfig *cfg, const float *K,
                        const PsMapBatch *b, const PsPairResults *out);

/* ---- N2 for FLOAT descriptors (SURF / SIFT): Matcher::matchXYZ with normType = cv::NORM_L2 on CV_32F rows
 * (matcher.cpp:625-628, :719-721, :737-739).  Candidates (sphere, level, ascending i), the emit rule, the record and its order
 * are ps_match_xyz's; only the VALUE of a candidate differs.  It is RESTATED from OpenCV 3.x's continuous path norm() ->
 * normL2_32f -> normL2Sqr<float, double>, not compiled against an OpenCV (tests/map_l2_ref.py):
 *   x[k] = (float)(map[k] - cur[k]) (cv::subtract on CV_32F); v[k] = (double)x[k]; s = 0.0;
 *   s = s + (((v0 v0 + v1 v1) + v2 v2) + v3 v3) over the blocks of four, then s = s + v v per remaining element;
 *   value = (float)sqrt(s), a correctly rounded double square root narrowed once.
 * Best value (:714-727): the first candidate is taken whatever its value, a later one if value < bestVal.  So a NaN value at the
 * first candidate leaves bestVal NaN and the feature emits nothing; a NaN at a later candidate is ignored; +inf is an ordinary
 * value.  Every candidate with acceptRatio * (double)value <= (double)bestVal is emitted as DMatch(j, i, -1, value), ordered by
 * (j, i) (acceptRatio 0 with a +inf candidate: 0 * inf = NaN, not emitted).
 * Host pointers, synchronous.  Rows are dim floats wide, 1 <= dim <= PS_MAX_L2_DIM, with pitches in BYTES (>= dim x 4); limits
 * and errors as ps_match_l2_f32.  Returns PS_ERR_BAD_ARG with *nout = required capacity if cap is too small. */
int ps_match_xyz_l2_f32(PsContext *ctx, const float *mapPos, const float *mapDesc, size_t mapDescStepBytes, const int32_t *mapLevel,
                        int nmap, const float *curPos, const float *curDesc, size_t curDescStepBytes, const int32_t *curLevel,
                        int ncur, int dim, double sphereRadius, double acceptRatio, PsDMatch *out, int cap, int *nout);

/* PsMapBatch with float-descriptor sets (THE RULES of PsFrameSetF32 for either; pts is needed); maps.dim must equal frames.dim.
 * ps_map_views_l2_device writes `maps` and mapLevel from a resident PsMapStoreF32 (further down); a host may also fill them. */
typedef struct PsMapBatchF32 {
    PsFrameSetF32 maps;           /* "map views": desc = the descriptor chosen for each visible feature, pts = (float) casts of
                                     MapFeature::position in the camera frame, nkpts = features per view */
    const int32_t *mapLevel;      /* maps.numFrames x maps.maxKpts predicted levels */
    PsFrameSetF32 frames;         /* current frames: descriptors + back-projected points */
    const int32_t *curLevel;      /* frames.numFrames x frames.maxKpts */
    const int32_t *pairs;         /* P x 2 (map view, frame), device */
    int32_t P;
    int32_t maxMatches;           /* row capacity of out->matches / out->inlierMask for every pair */
    float radiusBound;            /* ps_map_sphere_bound(radius), used when radiusBoundPerPair is NULL */
    double acceptRatio;           /* used when acceptRatioPerPair is NULL */
    const float *radiusBoundPerPair;   /* device, P, or NULL */
    const double *acceptRatioPerPair;  /* device, P, or NULL */
} PsMapBatchF32;
size_t ps_abi_sizeof_map_batch_f32(void);

/* ps_match_xyz_device / ps_map_pairs_device for a PsMapBatchF32: the same contract -- device pointers, asynchronous on the
 * context's stream, nothing copied, no synchronisation; numMatches[p] = -(count) for a pair over maxMatches, which the estimator
 * sees without matches; a pair naming a view or a frame outside its set has no matches -- with the value above.  Pair p's list
 * is byte for byte ps_match_xyz_l2_f32's, and mask, pose and stats of ps_map_pairs_l2_device are byte for byte those of
 * ps_match_xyz_l2_f32 followed by ps_ransac_rigid3d with cfg->seed + p.
 * maxKpts above PS_MAX_KPTS, dim above PS_MAX_L2_DIM, maxMatches above 1 << 22 -> PS_ERR_UNSUPPORTED; dim < 1, maps.dim !=
 * frames.dim, maxMatches < 1, a bad stride, NULL where an array is needed, P < 0 -> PS_ERR_BAD_ARG; outputs are not touched.
 * P == 0 is PS_OK.  Scratch as the binary calls (16 B a match of staging, about 150 B a match of records), shared with them. */
int ps_match_xyz_l2_device(PsContext *ctx, const PsMapBatchF32 *b, PsDMatch *matches, int32_t *numMatches);
int ps_map_pairs_l2_device(PsContext *ctx, const PsRansacParams *params, const PsRansacConfig *cfg, const float *K,
                           const PsMapBatchF32 *b, const PsPairResults *out);

/* ---- Map views built on the device from a RESIDENT feature map: what a host does per frame and per visible map feature before
 * matchXYZ -- FeaturesMap::findNearestFrame (src/Map/featuresMap.cpp:528-563), PUTSLAM::removeMapFeaturesWithoutGoodObservationAngle
 * (src/PUTSLAM/PUTSLAM.cpp:932-950), moveMapFeaturesToLocalCordinateSystem (PUTSLAM.cpp:28-51), the predicted level of
 * matcher.cpp:681-692 and the copy of the chosen descriptor (:675-679) -- for V views in one launch chain.  The output IS a
 * PsFrameSet + mapLevel, what PsMapBatch::maps / mapLevel read.
 *
 * The level without a device log: clamp(ceil(log(x) / log 1.2), 0, 7) is an integer decision in one monotone variable.
 * ps_level_thresholds: t[k], k = 0 .. 6, the least double with ceil(log(x) / log(1.2)) > k, found by bisection over bit patterns
 * with the host's libm evaluated exactly as ps_predicted_level evaluates it; the predicate is then checked to be clean -- true
 * from t[k] on, false below -- for every double within 4096 ulps of each t[k]: PS_ERR_UNSUPPORTED if it is not (a libm that is
 * not locally monotone: nothing is guessed).  Pure host arithmetic, no context.
 * THE LEVEL RULE of the two device calls below:  x = (T[octave] * detDist) / curDist  in double, left to right, with
 * T[o] = pow(1.2, o) from a host-filled table for o = PS_LEVEL_OCTAVE_MIN .. PS_LEVEL_OCTAVE_MAX; level = #{k : x >= t[k]} if x
 * is finite, else 0 -- what ps_predicted_level returns, NaN, +-inf, 0 and negative x included.  An octave outside the table never
 * gives a silent level: it invalidates the view (ps_map_views_device) or writes -1 (ps_frame_levels_device). */
#define PS_LEVEL_OCTAVE_MIN (-16)
#define PS_LEVEL_OCTAVE_MAX 47
int ps_level_thresholds(double t[7]);

/* The angle table of featuresMap.cpp:534-556 for one current pose: featureGlob there has an identity rotation, so
 * featureGlob.inverse() * camPose has camPose's rotation and the "view vector" is the pose's third rotation column whatever the
 * feature -- the angle depends on the pair (historical pose, current pose) only.  curPose16 / poses16: column-major 4x4 doubles
 * (Mat34 storage).  For pose q: a = float casts of the current pose's elements (0,2), (1,2), (2,2), b = those of pose q;
 * float dot = a0*b0 + (a1*b1 + a2*b2) and the two float norms in the same order (Eigen's Vector3f reductions as DESIGN.md 8.2
 * reads them) with a correctly rounded sqrtf; r = dot / (nb * na) in float; angle[q] = fabs(acos((double)r)) -- the DOUBLE acos
 * (whether the reference's unqualified acos on a float picks the float overload depends on its headers: DESIGN.md 8.4; the table
 * is an INPUT of ps_map_views_device, a host with the real build can supply its own).  Pure host arithmetic (libm). */
int ps_view_angles(const double *curPose16, const double *poses16, int numPoses, double *angle);

typedef struct PsMapStore {       /* DEVICE pointers: what FeaturesMap's front-end map holds */
    const double  *pos;           /* F x 3, MapFeature::position, global frame */
    const int32_t *obsStart;      /* F + 1: feature f's observations, ascending poseId
                                     (the order of std::map<poseId, ExtendedDescriptor>) */
    const int32_t *obsPose;       /* O, 0 .. numPoses-1 */
    const uint8_t *obsDesc;       /* O x 32, 16-byte aligned */
    const int32_t *obsOctave;     /* O */
    const double  *obsDetDist;    /* O */
    int32_t numFeatures, numObs, numPoses, reserved;
} PsMapStore;

enum { PS_VIEW_REQUIRE_VISIBLE = 1 };
typedef struct PsMapViewRequest { /* pointers: DEVICE */
    const double *camInv;         /* V x 16 column-major: cameraPose.inverse().matrix() (the caller inverts) */
    const double *poseAngle;      /* V x numPoses: ps_view_angles of each view's pose */
    const int32_t *cand;          /* V x candCapacity feature indices (the std::set order of getCovisibleFeatures), or NULL =
                                     every feature of the store in index order */
    const int32_t *candCounts;    /* V, 0 .. candCapacity (read only when cand is given) */
    double maxAngle;
    double fx, fy, cx, cy, imageW, imageH;   /* DepthSensorModel's focalLength / focalAxis / imageSize */
    int32_t V, candCapacity;
    int32_t flags;                /* PS_VIEW_REQUIRE_VISIBLE */
    int32_t reserved;
} PsMapViewRequest;

typedef struct PsMapViewOut {     /* pointers: DEVICE, written by the call */
    PsFrameSet views;             /* desc / pts / nkpts as a PsFrameSet of numFrames >= V views (dense or ABI 2 strides),
                                     maxKpts <= PS_MAX_KPTS: drops into PsMapBatch::maps */
    int32_t *mapLevel;            /* numFrames x maxKpts: PsMapBatch::mapLevel */
    int32_t *viewCount;           /* V, see below */
    /* side arrays for the host, each V x maxKpts rows or NULL: */
    int32_t *featIdx;             /* the feature */
    int32_t *obsIdx;              /* the chosen observation (index into the store's obs arrays) */
    double *posCam;               /* x 3: position in the camera frame */
    double *uv;                   /* x 2: MapFeature::u / v (-1, -1 when not visible) */
    double *angle;                /* angles[] of findNearestFrame */
} PsMapViewOut;
size_t ps_abi_sizeof_map_store(void);
size_t ps_abi_sizeof_map_view_request(void);
size_t ps_abi_sizeof_map_view_out(void);

/* For view v and candidate f, in candidate order:
 *  1. observation choice (featuresMap.cpp:537-561): f's observations are walked in order, the first with angle < best is kept
 *     (strict; best starts at 10; a NaN angle is never chosen); f is dropped if none is chosen or if the chosen angle is
 *     > maxAngle (equality keeps it);
 *  2. camera-frame position (PUTSLAM.cpp:35-40), M = camInv of v: p_i = ((M(i,0)*x + M(i,1)*y) + M(i,2)*z) + M(i,3) in double,
 *     every product and sum rounded (Eigen's fixed 4x4 product in a build without FMA);
 *  3. projection (depthSensorModel.cpp:18-25): u = ((fx*p0)/p2) + cx, v = ((fy*p1)/p2) + cy, both -1 if
 *     u<0 || u>imageW || v<0 || v>imageH || p2<0.8 || p2>6.0 (NaNs fall through); with PS_VIEW_REQUIRE_VISIBLE a feature whose
 *     u == -1 is dropped (featuresMap.cpp:471-474 without the lifeValue bookkeeping, which stays with the host);
 *  4. level (matcher.cpp:681-692): curDist = sqrt((p0*p0 + p1*p1) + p2*p2) in double, then the level rule with the chosen
 *     observation's octave and detDist;
 *  5. the next row of view v receives pts = float casts of p (:700-701), desc = the chosen observation's 32 bytes, mapLevel, and
 *     the side arrays.
 * views.nkpts[v] = viewCount[v] = the count.  If it exceeds maxKpts: viewCount[v] = -(count), nkpts[v] = 0, the rows need not be
 * meaningful, other views are unaffected (the rule of numMatches above; call again with that capacity).  viewCount[v] = INT32_MIN,
 * nkpts[v] = 0 for a view with a candidate count outside 0 .. candCapacity, a candidate index outside the store, a pose id
 * outside 0 .. numPoses-1 among a candidate's observations, an obsStart range that is not ascending inside 0 .. numObs, or an
 * EMITTED feature whose chosen observation's octave lies outside the table.  Rows beyond the count are not written.
 * Asynchronous on the context's stream, copies nothing and does not synchronise (growing scratch on a first call aside: 36 bytes
 * per view and 256 candidate slots).  NULL where an array is needed, a negative count, views.numFrames < V, maxKpts < 1, bad
 * strides -> PS_ERR_BAD_ARG (text: ps_last_error); maxKpts > PS_MAX_KPTS -> PS_ERR_UNSUPPORTED; outputs untouched.  V == 0 is
 * PS_OK.  Out of scope: incremental updates of the store (it is replaced whole), the covisibility walk, lifeValue, the inverse. */
int ps_map_views_device(PsContext *ctx, const PsMapStore *store, const PsMapViewRequest *req, const PsMapViewOut *out);

/* The frame side, matcher.cpp:639-652: curLevel[f][i] for the keypoints of a device-resident frame set.  octave / detDist /
 * curLevel: numFrames x maxKpts (rows beyond nkpts[f] are not written).  curDist = (double)sqrtf(p0*p0 + (p1*p1 + p2*p2)) in
 * float (Vector3f::norm), then the level rule.  An octave outside the table writes -1, never a level: the caller checks for it
 * (ps_match_xyz's test |curLevel - mapLevel| <= 1 fails for such a keypoint against map levels 1 .. 7, but NOT against map
 * level 0 -- a -1 must not reach the matcher unexamined).  Asynchronous, no scratch. */
int ps_frame_levels_device(PsContext *ctx, const PsFrameSet *frames, const int32_t *octave, const double *detDist,
                           int32_t *curLevel);

/* ---- Pyramidal Lucas-Kanade feature tracking: MatcherOpenCV::performTracking, src/Matcher/matcherOpenCV.cpp:209-300, the first
 * step of Matcher::trackKLT (src/Matcher/matcher.cpp:133-449) -- cv::calcOpticalFlowPyrLK on the image pair (:232-238), the error
 * gate (:247-252), the too-close-by-error removal (:254-265) and the compaction into cv::DMatch(i, j, 0) (:267-290).
 * The arithmetic is the project's reading of OpenCV 3.x's lkpyramid.cpp, scalar path with float accumulators (DESIGN.md section
 * 8.9, restated in tests/klt_ref.py): integer pyramid and Scharr passes, 14-bit bilinear weights rounded half to even, the 2x2
 * matrix and the mismatch vector as float sums in window order.  SIMD builds of OpenCV sum in another order and may differ in
 * the last bits of those sums.  status starts at 1 and err at 0; err of a failed point that OpenCV leaves undefined is 0. */
enum { PS_KLT_USE_INITIAL_FLOW = 4, PS_KLT_GET_MIN_EIGENVALS = 8 }; /* cv::OPTFLOW_USE_INITIAL_FLOW / OPTFLOW_LK_GET_MIN_EIGENVALS */
typedef struct PsKltParams {
    double eps;              /* TermCriteria epsilon: clamped to 0 .. 10, then squared (OpenCVParams.eps, :222) */
    double minEigThreshold;  /* OpenCVParams.trackingMinEigThreshold (:238) */
    int32_t winSize;         /* square window, 3 .. 31 (OpenCVParams.winSize, :234-235) */
    int32_t maxLevels;       /* 0 .. 7 (OpenCVParams.maxLevels, :236) */
    int32_t maxCount;        /* TermCriteria maxCount: clamped to 0 .. 100 (OpenCVParams.maxIter, :221) */
    int32_t flags;           /* PS_KLT_USE_INITIAL_FLOW | PS_KLT_GET_MIN_EIGENVALS (:225-229) */
} PsKltParams;
typedef struct PsImageSet {  /* numFrames interleaved 8-bit images of one shape; pixels: DEVICE */
    const uint8_t *pixels;
    size_t rowStride;        /* bytes between rows, 0 = dense (cols x channels) */
    size_t frameStride;      /* bytes between frames, 0 = dense (rows x rowStride) */
    int32_t numFrames, rows, cols, channels; /* channels 1 or 3 (the reference passes rgbImage) */
} PsImageSet;
typedef struct PsKltPyramids PsKltPyramids; /* a set of `slots` image pyramids with their derivatives, device resident */
size_t ps_abi_sizeof_klt_params(void);
size_t ps_abi_sizeof_image_set(void);

/* cv::buildOpticalFlowPyramid's storage for `slots` images of rows x cols x channels (what calcOpticalFlowPyrLK builds for its two
 * images, :232): level 0 and up to maxLevels reduced levels -- building stops before a level whose width or height would be
 * <= winSize -- each stored with its winSize-wide border (REFLECT_101 for the image, 0 for the derivative).
 * winSize 3 .. 31, maxLevels 0 .. 7, channels 1 or 3, slots 1 .. 65535, rows and cols above winSize, else PS_ERR_BAD_ARG; rows or
 * cols above 8192: PS_ERR_UNSUPPORTED.  Synchronous (allocates).  destroy waits for the device; NULL is harmless. */
int ps_klt_pyramids_create(PsContext *ctx, int rows, int cols, int channels, int winSize, int maxLevels, int slots, PsKltPyramids **out);
void ps_klt_pyramids_destroy(PsKltPyramids *pyr);
int ps_klt_pyramids_num_levels(const PsKltPyramids *pyr); /* levels stored, level 0 included; -1 for NULL */
/* Fills the levels and derivatives of slots firstSlot .. firstSlot + images->numFrames - 1 from device-resident images of the
 * set's shape: one launch per level and pass over all frames.  A shape other than the set's, a stride below its row / frame or
 * slots outside the set: PS_ERR_BAD_ARG.  Asynchronous on the context's stream; uses no scratch of the context. */
int ps_klt_pyramids_build_device(PsContext *ctx, PsKltPyramids *pyr, const PsImageSet *images, int firstSlot);
/* cv::calcOpticalFlowPyrLK (:232-238) for P pairs of slots: pairs P x 2 int32 (previous slot, next slot; a pair may name one slot
 * twice), prevPts / nextPts P x capacity x 2 floats, counts P int32, status P x capacity bytes, err P x capacity floats -- all
 * DEVICE.  nextPts is read only under PS_KLT_USE_INITIAL_FLOW.  params->winSize must be the set's; the level count is the
 * set's.  Nothing beyond a pair's count is written; a pair whose count lies outside 0 .. capacity is left alone altogether (the
 * count -1 of ps_dbscan_thin_device: ps_klt_select_device reports it); a pair that names a slot outside the set has its points
 * failed (status 0, err 0, nextPts untouched).  One wavefront per point.  Asynchronous; uses no scratch of the context. */
int ps_klt_track_device(PsContext *ctx, const PsKltPyramids *pyr, const PsKltParams *params, const int32_t *pairs, const float *prevPts,
                        const int32_t *counts, int P, int capacity, float *nextPts, uint8_t *status, float *err);
/* The selection (:247-290) for P pairs: a point survives iff status != 0, not (double)err > trackingErrorThreshold, and no i < j
 * sweep marked it -- for every pair of points, failed ones included, with sqrt((double)dx*dx + (double)dy*dy) <
 * minimalReprojDistance (float differences; decided as sum < ps_sqrt_bound_f64(distance)) i is marked if err[i] > err[j], else j;
 * a comparison that involves a NaN is false.  Survivor j (index order) of pair p: matches[p][j] = (i, j, 0, 0.f), keptPts[p][j]
 * its point, keptIdx[p][j] = i (what the caller compacts keyPoints / detDists with); numMatches[p] their number, -1 for a count
 * outside 0 .. capacity.  All arrays DEVICE, P x capacity; the inputs are not changed.  capacity <= PS_MAX_KPTS.  Asynchronous. */
int ps_klt_select_device(PsContext *ctx, const float *nextPts, const uint8_t *status, const float *err, const int32_t *counts, int P,
                         int capacity, double trackingErrorThreshold, double minimalReprojDistance, PsDMatch *matches,
                         int32_t *numMatches, float *keptPts, int32_t *keptIdx);
/* cv::calcOpticalFlowPyrLK(prevImg, nextImg, prevPts, nextPts, status, err, Size(winSize, winSize), maxLevels, criteria, flags,
 * minEigThreshold) (:232-238) for one pair: HOST pointers, uploads included, synchronous.  Images rows x cols x channels bytes,
 * rowStride bytes apart (0 = dense); nextPts is read under PS_KLT_USE_INITIAL_FLOW and written for all n points. */
int ps_calc_optical_flow_pyr_lk(PsContext *ctx, const uint8_t *prevImg, const uint8_t *nextImg, int rows, int cols, int channels,
                                size_t rowStride, const float *prevPts, float *nextPts, int n, uint8_t *status, float *err,
                                const PsKltParams *params);
/* MatcherOpenCV::performTracking (:209-300) for one pair, track + select: HOST pointers, synchronous.  nextPts (all n tracked
 * positions), status and err (either may be NULL) as above; matches / keptPts / keptIdx have room for n entries, *numMatches
 * receives the survivors' number.  n <= PS_MAX_KPTS. */
int ps_perform_tracking(PsContext *ctx, const uint8_t *prevImg, const uint8_t *nextImg, int rows, int cols, int channels, size_t rowStride,
                        const float *prevPts, float *nextPts, int n, const PsKltParams *params, double trackingErrorThreshold,
                        double minimalReprojDistance, uint8_t *status, float *err, PsDMatch *matches, int *numMatches, float *keptPts,
                        int32_t *keptIdx);
/* Diagnostic (no reference counterpart): one stored level of one slot read back to the HOST.  dims4 = {rows, cols, stored rows,
 * stored cols} (stored = with the border); img stored rows x stored cols x channels bytes; der the same elements as int16 pairs
 * (Ix, Iy).  Any of the three may be NULL.  Waits for the context's stream. */
int ps_debug_klt_level(PsContext *ctx, const PsKltPyramids *pyr, int slot, int level, int32_t *dims4, uint8_t *img, int16_t *der);

/* ---- FAST-9/16 key point detection: MatcherOpenCV::detectFeatures, src/Matcher/matcherOpenCV.cpp:118-180, for detector = "FAST"
 * (cv::FastFeatureDetector::create(), :64-65) -- the first step of the refill chain of Matcher::trackKLT (matcher.cpp:213-260):
 * cvtColor(RGB2GRAY) (:122), the grid of ROIs (:127-146), the detector in every ROI (:148), the per-ROI ordering by response and
 * cut to maximalTrackedFeatures * 3 / (gridCols * gridRows) (:155-165), the joined ordering and cut (:169-177).
 * The arithmetic is the project's reading of OpenCV 3.x's fast.cpp / fast_score.cpp (FAST_t<16>, cornerScore<16>) and of the 8-bit
 * cvtColor (restated twice in tests/fast_ref.py); no OpenCV build was at hand to pin it against.  All of
 * it is integer arithmetic, on which OpenCV's SIMD and scalar builds agree:
 *   grey      (c0 * 4899 + c1 * 9617 + c2 * 1868 + 8192) >> 14 -- channel 0 takes the red weight whatever the host stored there
 *             (the reference hands its BGR-loaded image to CV_RGB2GRAY as it is); channels == 1: the image is grey already (an
 *             extension for hosts that convert themselves, OpenCV would throw);
 *   ROIs      for k in 0 .. gridCols-1 (outer), i in 0 .. gridRows-1 (inner): origin (k * cols / gridCols, i * rows / gridRows),
 *             size cols / gridCols x rows / gridRows, integer divisions: a remainder strip is never looked at.  The detector sees
 *             an ROI as an image of its own: candidates are its rows 3 .. R-4 and columns 3 .. C-4 (R or C < 7: none);
 *   corner    with d[k] = v - ring[k] over the ring (0,3) (1,3) (2,2) (3,1) (3,0) (3,-1) (2,-2) (1,-3) (0,-3) (-1,-3) (-2,-2) (-3,-1)
 *             (-3,0) (-3,1) (-2,2) (-1,3): nine cyclically consecutive d all > t or all < -t, t = threshold clamped to 0 .. 255;
 *   score     max(t, D, B) - 1 as a byte, D = the largest over the 16 arcs of nine of the least d, B the same for -d; 0 for a
 *             non-corner;
 *   emission  with suppression: a corner whose score is strictly above its eight neighbours' (two equal neighbours suppress
 *             each other, a corner of score 0 -- t = 0 only -- never comes out), response = score; without: every corner,
 *             response 0 (OpenCV computes no score in that mode);
 *   order     THE ONE PLACE this library decides what the reference leaves open: both orderings by response are std::sort with
 *             p1.response > p2.response (matcherOpenCV.h:84-87), which is not stable, so among equal responses the reference's
 *             order -- and who survives a cut that falls inside a tie -- is whatever its libstdc++ does.  Here both are STABLE:
 *             ties keep raster order (y, then x) inside an ROI and the order of the ROI loop across ROIs.
 * A key point is (pt = (x, y) in image coordinates, size 7, angle -1, response, octave 0, class_id -1); the calls return pt and
 * response. */
typedef struct PsDetectParams {
    int32_t threshold;               /* clamped to 0 .. 255; FastFeatureDetector::create(): 10 */
    int32_t nonmaxSuppression;       /* 0 = off; create(): on */
    int32_t gridRows, gridCols;      /* OpenCVParams.gridRows / gridCols, at least 1 */
    int32_t maximalTrackedFeatures;  /* OpenCVParams.maximalTrackedFeatures, 0 .. PS_MAX_KPTS */
    int32_t reserved;                /* must be 0 */
} PsDetectParams;
typedef struct PsFastDetector PsFastDetector; /* grey, score and corner maps for up to maxFrames images of one shape, device resident */
size_t ps_abi_sizeof_detect_params(void);

/* A detector for images of rows x cols x channels bytes, up to maxFrames (1 .. 65535) a call: three byte planes per frame.
 * rows or cols < 1, channels other than 1 or 3, maxFrames outside its range -> PS_ERR_BAD_ARG; rows or cols above 8192 ->
 * PS_ERR_UNSUPPORTED.  Synchronous (allocates).  destroy waits for the device; NULL is harmless. */
int ps_fast_detector_create(PsContext *ctx, int rows, int cols, int channels, int maxFrames, PsFastDetector **out);
void ps_fast_detector_destroy(PsFastDetector *det);
/* detectFeatures for every frame of a device-resident set (the PsImageSet the KLT pyramids are built from).  xy numFrames x
 * capacity x 2 floats, response numFrames x capacity floats, counts numFrames int32 -- all DEVICE; frame f's counts[f] key points
 * fill its first rows in the final order, nothing beyond them is written.  The layout is the one ps_dbscan_thin_device takes
 * (octave = NULL) and whose kept indices ps_klt_track_device's callers gather with: no repacking step in between.
 * Three launches whatever the frame count: the score pass over all frames, one work-group per (frame, ROI) that orders and cuts
 * the ROI, one per frame that joins them.  Asynchronous on the context's stream, except that a call which needs more room for
 * its ROI lists than any call before (4 bytes per kept key point of every ROI) allocates first, which waits for the device.
 * NULL where an array is needed, gridRows / gridCols < 1, maximalTrackedFeatures < 0, reserved != 0, a shape or stride that does
 * not fit the detector, numFrames < 0 or above maxFrames, capacity < min(maximalTrackedFeatures, candidate pixels of all ROIs)
 * -> PS_ERR_BAD_ARG (text: ps_last_error); maximalTrackedFeatures or capacity above PS_MAX_KPTS -> PS_ERR_UNSUPPORTED; outputs
 * untouched.  numFrames == 0 is PS_OK. */
int ps_detect_features_device(PsContext *ctx, PsFastDetector *det, const PsImageSet *images, const PsDetectParams *params, int capacity,
                              float *xy, float *response, int32_t *counts);
/* detectFeatures for one image: HOST pointers, upload included, synchronous.  img rows x cols x channels bytes, rowStride bytes
 * between rows (0 = dense; a region of a larger image keeps its parent's).  xy cap x 2 floats, response cap floats, *nout the
 * number found.  Returns PS_ERR_BAD_ARG with *nout = required capacity if cap is too small (nothing else is written); other
 * errors as above, *nout untouched. */
int ps_detect_features(PsContext *ctx, const uint8_t *img, int rows, int cols, int channels, size_t rowStride, const PsDetectParams *params,
                       float *xy, float *response, int cap, int *nout);
/* Diagnostic (no reference counterpart): the grey image, the score map and the corner map (1 = corner) of one frame of the
 * detector's LAST call read back to the HOST, rows x cols bytes each; any of the three may be NULL.  Waits for the context's
 * stream. */
int ps_debug_fast_maps(PsContext *ctx, const PsFastDetector *det, int frame, uint8_t *gray, uint8_t *score, uint8_t *corner);
/* Diagnostic (no reference counterpart; profiles/scripts/fast_times.py times each pass alone with it): ps_detect_features_device
 * with only the passes of the mask queued -- 1 the score pass, 2 the per-ROI selection, 4 the join.  A pass reads what the passes
 * before it left in the detector: call with 7 (= ps_detect_features_device) and the same arguments first. */
int ps_debug_fast_passes(PsContext *ctx, PsFastDetector *det, const PsImageSet *images, const PsDetectParams *params, int capacity,
                         float *xy, float *response, int32_t *counts, int passes);

/* ---- ORB descriptor extraction: MatcherOpenCV::describeFeatures, src/Matcher/matcherOpenCV.cpp:183-195, for descriptor = "ORB"
 * (descriptorExtractor->compute(rgbImage, features, descriptors) with cv::ORB::create()) -- the last per-frame step of
 * Matcher::detectInitFeatures (matcher.cpp:36), Matcher::match (:467) and Matcher::trackKLT (:338).  The rows are the 32-byte rows
 * ps_match_hamming256, ps_match_xyz* and the resident map store take.
 * The arithmetic is the project's reading of OpenCV 3.0 - 3.3's ORB_Impl::detectAndCompute with useProvidedKeypoints = true: orb.cpp,
 * the 8-bit resize(INTER_LINEAR), the 8-bit separable GaussianBlur and cvtColor (restated twice in
 * tests/orb_ref.py); no OpenCV build was at hand to pin it against -- the reading is UNPINNED.  ORB's sampling pattern is DATA
 * here: a host that wants OpenCV's rows passes OpenCV's 256 x 4 table, NULL selects the documented default below.  Everything but
 * the rotation is integer arithmetic; cvRound rounds half to even; float operations are single IEEE operations:
 *   grey      1 channel: the image as it is.  3 channels: COLOR_BGR2GRAY, (c0 * 1868 + c1 * 9617 + c2 * 4899 + 8192) >> 14 -- not
 *             the detector's RGB2GRAY weights: in the reference the same buffer goes through both conversions;
 *   levels    for l in 0 .. nLevels-1: scale_l = (float)pow((double)scaleFactor, l), rows_l = cvRound((float)rows / scale_l), cols_l
 *             alike; level 0 is the grey image, level l is resized from level l - 1 (480 x 640, 1.2: 400 x 533, 333 x 444, ...);
 *   resize    per destination index d of an axis with sn source and dn destination pixels: scale = 1.0 / ((double)dn / sn),
 *             f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= s; columns: s < 0 -> s = 0, f = 0; s >= sn-1 -> s = sn-1,
 *             f = 0; rows keep f and clamp the indices s, s + 1 to 0 .. sn-1; a0 = cvRound((1.f - f) * 2048.f), a1 =
 *             cvRound(f * 2048.f).  h = S[s] * a0 + S[min(s+1, sn-1)] * a1 (int), out = (((b0 * (h0 >> 4)) >> 16) +
 *             ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
 *   blur      7 x 7, sigma 2, integer taps {18, 34, 49, 55, 49, 34, 18} = cvRound(256 g): they sum to 257, which is part of the
 *             reading (a constant 128 blurs to 129).  Rows first, then columns, in int; out = min(255, (v + 32768) >> 16);
 *             BORDER_REFLECT_101 of the unblurred level as cv::borderInterpolate does it: a length of 1 gives index 0, else
 *             p < 0 -> -p, p >= n -> 2n - 2 - p, repeated until inside.  Every level is kept raw and blurred;
 *   kept      a key point is described iff 31 <= x < cols-31, 31 <= y < rows-31 (float compares, NaN fails; rows or cols <= 62:
 *             none) and 0 <= octave < nLevels (an extension: OpenCV would index out of bounds).  The kept ones are grouped by
 *             octave ascending and keep their input order inside an octave (OpenCV's !sortedByLevel branch; what trackKLT
 *             :302-331 does by hand); keptIdx[j] is the input index of output row j;
 *   row       s = 1.f / scale_octave; centre (cvRound(x * s), cvRound(y * s)) in that level; (a, b) = (cos, sin) of angle degrees;
 *             for a pattern point (px, py): ix = cvRound(px * a - py * b), iy = cvRound(px * b + py * a); bit p of the row -- byte
 *             p >> 3, bit p & 7 -- is v(point 0) < v(point 1) of pair p.  v reads the blurred level where the pixel lies inside the
 *             level and the RAW level at the REFLECT_101 index where it lies outside (OpenCV blurs a region of an atlas in place:
 *             the border around the region holds unblurred reflected copies);
 *   rotation  one fixed float sequence of this library's own (cosf differs between libraries), no fused operation: an angle that is
 *             not finite or beyond 2^20 in magnitude counts as 0; q = rint(angle * (float)(1 / 90.)), r = angle - q * 90.f (exact),
 *             k = (int)q & 3, t = r * (float)(pi / 180), u = t * t; S = ((((S9 u + S7) u + S5) u + S3) (t u)) + t and
 *             C = (((((C10 u + C8) u + C6) u + C4) u + C2) u) + 1.f with Sn, Cn = (float)(+-1 / n!), every product and sum rounded
 *             on its own; (a, b) = (C, S), (-S, C), (-C, -S), (S, -C) for k = 0 .. 3.  Against float64 cos / sin the absolute
 *             error stays below 2^-20 (measured: 7.2e-8), so a sample differs from the exact rotation's only where its exact
 *             coordinate lies within 2^-15 px of a half-integer;
 *   pattern   256 pairs x (x0, y0, x1, y1) int8, every coordinate in -15 .. 15.  The default: SplitMix64 from state
 *             0x5055545F4F5242 (add 0x9E3779B97F4A7C15; z ^= z >> 30, z *= 0xBF58476D1CE4E5B9; z ^= z >> 27, z *=
 *             0x94D049BB133111EB; z ^= z >> 31); per draw u, coordinate i is ((u >> 8i) & 15) + ((u >> (8i + 4)) & 15) - 15; a
 *             draw whose two points are equal is drawn again.  It starts (11,-7,-5,-7) (-7,0,-2,-1) (-8,-3,5,-8) (-8,0,-12,-6). */
typedef struct PsOrbParams {
    float scaleFactor;    /* 1 < scaleFactor <= 2; cv::ORB::create(): 1.2f */
    int32_t nLevels;      /* 1 .. 8; create(): 8 */
    int32_t reserved[2];  /* must be 0 */
} PsOrbParams;
typedef struct PsOrbPyramids PsOrbPyramids; /* `slots` image pyramids, every level raw and blurred, with the pattern; device resident */
size_t ps_abi_sizeof_orb_params(void);
/* The default pattern, 1024 int8 (pure host arithmetic, no context); PS_ERR_BAD_ARG for NULL. */
int ps_orb_pattern_default(int8_t *out1024);

/* Storage for `slots` (1 .. 65535) pyramids of rows x cols x channels images, the resize coefficients (built once, here) and the
 * pattern: pattern1024 is a HOST array of 256 x 4 int8, NULL = the default.  A NULL argument, a parameter outside its range, an
 * empty level, channels other than 1 or 3, a pattern coordinate outside -15 .. 15 -> PS_ERR_BAD_ARG; rows or cols above 8192 ->
 * PS_ERR_UNSUPPORTED.  Synchronous (allocates).  destroy waits for the device; NULL is harmless. */
int ps_orb_pyramids_create(PsContext *ctx, int rows, int cols, int channels, const PsOrbParams *params, const int8_t *pattern1024, int slots,
                           PsOrbPyramids **out);
void ps_orb_pyramids_destroy(PsOrbPyramids *pyr);
/* dims2 = {rows, cols} and the scale of one level (either may be NULL); PS_ERR_BAD_ARG for NULL or no such level.  No context. */
int ps_orb_pyramids_level(const PsOrbPyramids *pyr, int level, int32_t *dims2, float *scale);
/* Fills slots firstSlot .. firstSlot + images->numFrames - 1 from device-resident images of the set's shape (the PsImageSet the
 * KLT pyramids and the detector take): one launch per level and pass over all frames.  A shape other than the set's, a stride
 * below its row / frame or slots outside the set: PS_ERR_BAD_ARG.  Asynchronous on the context's stream. */
int ps_orb_pyramids_build_device(PsContext *ctx, PsOrbPyramids *pyr, const PsImageSet *images, int firstSlot);
/* describeFeatures for F frames: frame f's key points are rows 0 .. counts[f]-1 of xy (F x capacity x 2 floats), angle (F x capacity
 * floats, degrees), octave (F x capacity int32) -- the layout of ps_detect_features_device and ps_klt_select_device -- and are
 * described in the pyramid of slot slots[f] (two frames may name one slot).  desc F x capacity x 32 bytes, keptIdx F x capacity
 * int32, numKept F int32; all arrays DEVICE.  Frame f's numKept[f] rows come out in the order above; nothing is written beyond
 * them.  A frame whose count lies outside 0 .. capacity gets numKept[f] = -1 and nothing else; one that names a slot outside the
 * set gets numKept[f] = 0 and nothing else.  Two launches: a work-group per frame places the key points, a wavefront per kept key
 * point writes its row.  NULL where an array is needed, capacity < 1, F outside 0 .. 65535 -> PS_ERR_BAD_ARG; capacity above
 * PS_MAX_KPTS -> PS_ERR_UNSUPPORTED; F == 0 is PS_OK.  Asynchronous; uses no scratch of the context. */
int ps_describe_features_device(PsContext *ctx, const PsOrbPyramids *pyr, const int32_t *slots, const float *xy, const float *angle,
                                const int32_t *octave, const int32_t *counts, int F, int capacity, uint8_t *desc, int32_t *keptIdx,
                                int32_t *numKept);
/* describeFeatures for one image: HOST pointers, uploads included, synchronous.  img rows x cols x channels bytes, rowStride bytes
 * between rows (0 = dense); n key points (n <= PS_MAX_KPTS, else PS_ERR_UNSUPPORTED); desc n x 32 bytes and keptIdx n int32 receive
 * the *nout kept rows.  Errors as above, outputs untouched. */
int ps_describe_features(PsContext *ctx, const uint8_t *img, int rows, int cols, int channels, size_t rowStride, const PsOrbParams *params,
                         const int8_t *pattern1024, const float *xy, const float *angle, const int32_t *octave, int n, uint8_t *desc,
                         int32_t *keptIdx, int *nout);
/* Diagnostic (no reference counterpart): the raw and the blurred plane of one level of one slot read back to the HOST, rows_l x
 * cols_l bytes each (ps_orb_pyramids_level); either may be NULL.  Waits for the context's stream. */
int ps_debug_orb_level(PsContext *ctx, const PsOrbPyramids *pyr, int slot, int level, uint8_t *raw, uint8_t *blurred);
/* Diagnostic (no reference counterpart; profiles/scripts/orb_times.py times each pass alone with it): the arguments of
 * ps_orb_pyramids_build_device and ps_describe_features_device with only the passes of the mask queued -- 1 level 0, 2 the
 * resizes, 4 the blurs, 8 the placement, 16 the rows.  A pass reads what the passes before it left: call with 31 first.  The
 * build arguments are checked only if the mask names a build pass, the describe arguments only if it names one of theirs. */
int ps_debug_orb_passes(PsContext *ctx, PsOrbPyramids *pyr, const PsImageSet *images, int firstSlot, const int32_t *slots, const float *xy,
                        const float *angle, const int32_t *octave, const int32_t *counts, int F, int capacity, uint8_t *desc, int32_t *keptIdx,
                        int32_t *numKept, int passes);

/* ---- ORB key point detection: MatcherOpenCV::detectFeatures, src/Matcher/matcherOpenCV.cpp:118-180, for detector = "ORB"
 * (cv::ORB::create(), :66-67) -- the SHIPPED detector (resources/putslammatcherOpenCVParameters.xml:64) and the first per-frame step
 * of Matcher::match: cvtColor(RGB2GRAY) (:122), the grid of ROIs (:127-146), the detector in every ROI (:148), the per-ROI ordering
 * and cut (:155-165), the joined ordering and cut (:169-177).  The arrays it writes are the ones ps_dbscan_thin_device (with
 * octave) and ps_describe_features_device take.
 * The arithmetic is the project's reading of OpenCV 3.0 - 3.3's ORB_Impl::detectAndCompute (key points only), computeKeyPoints,
 * HarrisResponses, ICAngles, KeyPointsFilter and scalar fastAtan2 (restated twice in
 * tests/orb_detect_ref.py); no OpenCV build was at hand to pin it against -- the reading is UNPINNED.  Integer arithmetic except
 * where stated; float operations are single IEEE operations without contraction; cvRound rounds half to even:
 *   grey      the WHOLE image with CV_RGB2GRAY, (c0 * 4899 + c1 * 9617 + c2 * 1868 + 8192) >> 14 -- the FAST detector's weights, not
 *             the descriptor's; channels == 1: grey already;
 *   ROIs      the grid of the FAST section above; the detector sees an ROI as an image of its own, so every ROI has ITS OWN pyramid
 *             of rows / gridRows x cols / gridCols pixels.  Levels, scales and the resize are the ORB descriptor section's; only
 *             the raw levels are read, nothing is blurred;
 *   constants edgeThreshold 31, firstLevel 0, HARRIS_SCORE, patchSize 31 (cv::ORB::create()'s);
 *   quotas    factor = (float)(1.0 / scaleFactor); nd = nFeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)nLevels)) in
 *             float; for l = 0 .. nLevels-2: q_l = cvRound(nd), nd *= factor; q_last = max(nFeatures - sum q_l, 0)
 *             (500 / 1.2 / 8: 109 90 75 63 52 44 36 31);
 *   level l   FAST-9/16 with threshold fastThreshold (clamped to 0 .. 255) and suppression on the level as an image of its own,
 *             response = score; kept 31 <= x < cols_l - 31, 31 <= y < rows_l - 31 (rows_l or cols_l <= 62: nothing); retainBest(2 q_l)
 *             by the score: no more than n remain -> all stay, n = 0 -> none, else every key point whose response is >= the n-th
 *             largest stays: TIES AT THE CUT ARE ALL KEPT, so the surviving set is defined although nth_element's order is not;
 *   Harris    at the survivor's (x0, y0) in the raw level, block 7, k = 0.04f: over the 49 pixels p with row pitch s,
 *             Ix = (p[1] - p[-1]) * 2 + (p[-s+1] - p[-s-1]) + (p[s+1] - p[s-1]), Iy = (p[s] - p[-s]) * 2 + (p[s-1] - p[-s-1]) +
 *             (p[s+1] - p[-s+1]); int a = sum Ix^2, b = sum Iy^2, c = sum Ix Iy; scale = 1.f / (4 * 7 * 255.f), s4 = scale * scale *
 *             scale * scale (left to right); response = ((fa * fb - fc * fc) - (k * (fa + fb)) * (fa + fb)) * s4 with fa = (float)a
 *             ..., every operation rounded on its own; then retainBest(q_l) by this response, ties kept;
 *   angle     the intensity centroid over the disc of half patch 15: umax[0 .. 15] = 15 15 15 15 14 14 14 13 13 12 11 10 9 8 6 3,
 *             m10 = sum u I(u, v), m01 = sum v I(u, v) over |v| <= 15, |u| <= umax[|v|]; angle = fastAtan2((float)m01, (float)m10);
 *   fastAtan2 one fixed float sequence, degrees: ax = |x|, ay = |y|, c = min(ax, ay) / (max(ax, ay) + (float)DBL_EPSILON), c2 = c * c,
 *             a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c with p1, p3, p5, p7 = (float)0.9997878412794807, (float)-0.3258083974640975,
 *             (float)0.1555786518463281, (float)-0.04432655554792128, each times (float)(180 / pi); a = 90 - a if ax < ay; a = 180 - a
 *             if x < 0; a = 360 - a if y < 0; (0, 0) gives 0.  Within 0.0096 degrees of atan2 (measured; OpenCV documents 0.3);
 *   ROI list  levels ascending, raster order (y, then x) inside a level -- THIS ORDER IS THE LIBRARY'S DECISION, the reference's
 *             nth_element / partition leave it open; pt = (x0 * scale_l, y0 * scale_l) as float products, size 31 * scale_l,
 *             octave l, class_id -1, angle and the Harris response;
 *   order     the grid loop of the FAST section: both orderings STABLE by response > (descending floats, negative responses are
 *             ordinary), the cut to maximalTrackedFeatures * 3 / (gridCols * gridRows) per ROI, the ROI origin added as floats, the
 *             joined ordering, the cut to maximalTrackedFeatures. */
typedef struct PsOrbDetectParams {
    int32_t nFeatures;               /* 0 .. PS_MAX_KPTS; cv::ORB::create(): 500 */
    float scaleFactor;               /* 1 < scaleFactor <= 2; create(): 1.2f */
    int32_t nLevels;                 /* 1 .. 8; create(): 8 */
    int32_t fastThreshold;           /* clamped to 0 .. 255; create(): 20 */
    int32_t gridRows, gridCols;      /* OpenCVParams.gridRows / gridCols, at least 1 */
    int32_t maximalTrackedFeatures;  /* OpenCVParams.maximalTrackedFeatures, 0 .. PS_MAX_KPTS */
    int32_t reserved;                /* must be 0 */
} PsOrbDetectParams;
typedef struct PsOrbDetector PsOrbDetector; /* the pyramids (raw and FAST score planes) of every ROI of up to maxFrames images, and the lists */
size_t ps_abi_sizeof_orb_detect_params(void);
/* The per-level quotas of `params` (nFeatures, scaleFactor, nLevels), eight int32, 0 beyond nLevels.  Pure host arithmetic, no
 * context; PS_ERR_BAD_ARG for NULL or parameters outside their ranges. */
int ps_orb_detect_quotas(const PsOrbDetectParams *params, int32_t *quotas8);

/* A detector for images of rows x cols x channels bytes, up to maxFrames a call.  The grid, scaleFactor and nLevels of `params`
 * are fixed here: they shape the pyramids, one per (frame, ROI).  A NULL argument, a parameter outside its range, channels other
 * than 1 or 3, an empty ROI or level, maxFrames x gridRows x gridCols outside 1 .. 65535 -> PS_ERR_BAD_ARG; rows or cols above
 * 8192, nFeatures or maximalTrackedFeatures above PS_MAX_KPTS -> PS_ERR_UNSUPPORTED.  Synchronous (allocates).  destroy waits for
 * the device; NULL is harmless. */
int ps_orb_detector_create(PsContext *ctx, int rows, int cols, int channels, const PsOrbDetectParams *params, int maxFrames,
                           PsOrbDetector **out);
void ps_orb_detector_destroy(PsOrbDetector *det);
/* dims2 = {rows, cols} and the scale of one level of an ROI's pyramid (either may be NULL); PS_ERR_BAD_ARG for NULL or no such
 * level.  No context. */
int ps_orb_detector_level(const PsOrbDetector *det, int level, int32_t *dims2, float *scale);
/* detectFeatures for every frame of a device-resident set.  xy numFrames x capacity x 2 floats, response and angle numFrames x
 * capacity floats, octave numFrames x capacity int32, counts numFrames int32 -- all DEVICE; frame f's counts[f] key points fill its
 * first rows in the final order, nothing beyond them is written.  The layout is the one ps_dbscan_thin_device and
 * ps_describe_features_device take: no repacking step in between.  params: nFeatures, fastThreshold and maximalTrackedFeatures are
 * this call's; scaleFactor, nLevels, gridRows and gridCols must be the detector's.  Asynchronous on the context's stream, except
 * that a call which needs more room for its ROI lists than any call before allocates first, which waits for the device.
 * NULL where an array is needed, a parameter outside its range or other than the detector's, a shape or stride that does not fit
 * the detector, numFrames < 0 or above maxFrames, capacity < min(maximalTrackedFeatures, what the ROIs can emit) -> PS_ERR_BAD_ARG
 * (text: ps_last_error); nFeatures, maximalTrackedFeatures or capacity above PS_MAX_KPTS -> PS_ERR_UNSUPPORTED; outputs untouched.
 * numFrames == 0 is PS_OK. */
int ps_orb_detect_frames(PsContext *ctx, PsOrbDetector *det, const PsImageSet *images, const PsOrbDetectParams *params, int capacity,
                         float *xy, float *response, float *angle, int32_t *octave, int32_t *counts);
/* detectFeatures for one image: HOST pointers, upload included, synchronous.  img rows x cols x channels bytes, rowStride bytes
 * between rows (0 = dense; a region of a larger image keeps its parent's).  xy cap x 2 floats, response / angle cap floats, octave
 * cap int32, *nout the number found.  Returns PS_ERR_BAD_ARG with *nout = required capacity if cap is too small (nothing else is
 * written); other errors as above, *nout untouched. */
int ps_detect_features_orb(PsContext *ctx, const uint8_t *img, int rows, int cols, int channels, size_t rowStride,
                           const PsOrbDetectParams *params, float *xy, float *response, float *angle, int32_t *octave, int cap, int *nout);
/* Diagnostic (no reference counterpart): one level of one slot (slot = frame * gridRows * gridCols + ROI in loop order) of the
 * detector's LAST call read back to the HOST: the raw level and its FAST score plane, rows_l x cols_l bytes each; *numFirst the
 * survivors of the first cut, and the first min(*numFirst, cap) of them in raster order: yx = y << 16 | x, their Harris response and
 * angle, and kept = 1 where the second cut keeps them.  Any pointer may be NULL.  Waits for the context's stream. */
int ps_debug_orb_detect_level(PsContext *ctx, const PsOrbDetector *det, int slot, int level, uint8_t *raw, uint8_t *score, int32_t *numFirst,
                              uint32_t *yx, float *response, float *angle, uint8_t *kept, int cap);
/* Diagnostic (no reference counterpart; profiles/scripts/orb_detect_times.py times each pass alone with it): ps_orb_detect_frames
 * with only the passes of the mask queued -- 1 the pyramids, 2 the FAST scores, 4 the first cut, 8 Harris and angle, 16 the second
 * cut and the ROI ordering, 32 the join.  A pass reads what the passes before it left: call with 63 first. */
int ps_debug_orb_detect_passes(PsContext *ctx, PsOrbDetector *det, const PsImageSet *images, const PsOrbDetectParams *params, int capacity,
                               float *xy, float *response, float *angle, int32_t *octave, int32_t *counts, int passes);

/* ---- Frame assembly: what Matcher::detectInitFeatures (src/Matcher/matcher.cpp:17-64) and Matcher::match (:452-516) do between
 * "key points" and "descriptors with 3-D points": the DBScan survivors compacted (dbscan.run erases from the vector, :24-26), the
 * described key points undistorted and back-projected IN THE DESCRIBED ORDER (descriptorExtractor->compute replaces the vector,
 * :36-49) and the detection distances (:51-58) -- and the whole per-frame front end as one call on one stream, from a batch of
 * RGB-D images to a dense PsFrameSet. */
typedef struct PsDepthSet {  /* numFrames 16-bit depth images of one shape (PsImageSet's 16-bit twin); pixels: DEVICE */
    const uint16_t *pixels;
    size_t rowStride;        /* BYTES between rows, 0 = dense (cols x 2) */
    size_t frameStride;      /* BYTES between frames, 0 = dense (rows x rowStride); at least one view, also for a single frame */
    int32_t numFrames, rows, cols;
} PsDepthSet;
typedef struct PsFrameGeometry {
    float K[9];              /* camera matrix, row-major (cameraMatrixMat) */
    double dist5[5];         /* k1 k2 p1 p2 k3 (distortionCoeffsMat) */
    double depthImageScale;  /* sensorData.depthImageScale */
} PsFrameGeometry;
typedef struct PsFrameRowsOut {  /* DEVICE pointers, each F x capacity rows (nkpts: F); NULL = not wanted, except pts and nkpts */
    float *pts;              /* x 3: features3D -- with nkpts and the descriptors a dense PsFrameSet */
    int32_t *nkpts;
    float *xy;               /* x 2: the distorted position (prevFeaturesDistorted) */
    float *xyUndist;         /* x 2: prevFeaturesUndistorted */
    float *angle, *response; /* the key point's, from angleIn / responseIn */
    int32_t *octave;         /* ... from octaveIn */
    int32_t *srcIdx;         /* the input row this output row was taken from */
    double *detDist;         /* prevDetDists: what ps_frame_levels_device and the map store take */
    const float *angleIn, *responseIn; /* F x capacity, the layout of xy; needed where the output beside it is wanted */
    const int32_t *octaveIn;
} PsFrameRowsOut;
size_t ps_abi_sizeof_depth_set(void);
size_t ps_abi_sizeof_frame_geometry(void);
size_t ps_abi_sizeof_frame_rows_out(void);

/* Compacts F frames of key points by index lists (ps_dbscan_thin_device's keptIdx / nkept): output row j of frame f is input row
 * idx[f][j] for j < nidx[f], countsOut[f] = nidx[f].  All arrays DEVICE, F x capacity rows in the detector's layout (xy x 2 floats).
 * A frame whose nidx[f] lies outside 0 .. capacity gets countsOut[f] = -1 and nothing else (the convention of DBScan and of
 * describe: a bad frame propagates); an index outside 0 .. capacity-1 is not followed: that row is written as zeros.  Nothing is
 * written beyond a frame's count.  response / angle / octave are optional as In / Out PAIRS: both NULL = not wanted, one NULL ->
 * PS_ERR_BAD_ARG.  The outputs must not overlap the inputs.  NULL where an array is needed, capacity < 1, F outside 0 .. 65535 ->
 * PS_ERR_BAD_ARG; capacity above PS_MAX_KPTS -> PS_ERR_UNSUPPORTED; F == 0 is PS_OK.  One launch, asynchronous on the context's
 * stream; uses no scratch of the context. */
int ps_gather_keypoints(PsContext *ctx, const int32_t *idx, const int32_t *nidx, int F, int capacity, const float *xyIn,
                        const float *responseIn, const float *angleIn, const int32_t *octaveIn, float *xyOut, float *responseOut,
                        float *angleOut, int32_t *octaveOut, int32_t *countsOut);

/* For output row j < numKept[f] of frame f: i = keptIdx[f][j] (ps_describe_features_device's), p = xy[f][i]; undist = the
 * arithmetic of ps_remove_image_distortion on p; out->pts[f][j] = the arithmetic of ps_keypoints2Dto3D on undist in depth frame
 * firstDepthFrame + f -- frame g spans ps_depth_view_bytes(rows, cols, rowStride) bytes from pixels + g x frameStride, and the rule
 * of ps_keypoints2Dto3D holds for that frame alone AS THE DENSE IMAGE the reference holds: u == cols in a row that is not the last
 * reads the next row's first pixel whatever the row stride, u == cols in the last row and v == rows read depth 0.  A set's padding
 * is alignment, not a parent image: neither it nor the next frame is ever read.
 * out->nkpts[f] = numKept[f], or 0 where that lies outside 0 .. capacity (a frame set carries no negative count).  An index
 * outside 0 .. capacity-1 is not followed: every wanted array of that row is written as zeros.  detDist is matcher.cpp:52-57 as
 * the compiler sees it: float products, float sums left to right, no fused operation, the correctly rounded float square root,
 * then widened to double.  Nothing is written beyond a frame's count.  A NULL among geometry, depth, xy, keptIdx, numKept, out,
 * out->pts, out->nkpts or an input beside a wanted output, a depth set whose strides do not resolve, firstDepthFrame < 0 or firstDepthFrame + F above its numFrames, capacity < 1, F outside 0 .. 65535 ->
 * PS_ERR_BAD_ARG; capacity above PS_MAX_KPTS -> PS_ERR_UNSUPPORTED; F == 0 is PS_OK.  One launch, asynchronous; no scratch. */
int ps_assemble_frames(PsContext *ctx, const PsFrameGeometry *geometry, const PsDepthSet *depth, int firstDepthFrame, const float *xy,
                       const int32_t *keptIdx, const int32_t *numKept, int F, int capacity, const PsFrameRowsOut *out);

/* The per-frame front end for images of one shape, detector and descriptor "ORB": ps_orb_detect_frames, ps_dbscan_thin_device
 * (minPts 2, featuresFromCluster 1: dbscan.h:19), ps_gather_keypoints, ps_orb_pyramids_build_device, ps_describe_features_device
 * and ps_assemble_frames on the context's stream, with no host step in between. */
typedef struct PsFrontEndParams {
    PsOrbDetectParams detect;
    PsOrbParams describe;
    double DBScanEps;        /* OpenCVParams.DBScanEps */
} PsFrontEndParams;
typedef struct PsFrontEnd PsFrontEnd; /* a PsOrbDetector, a PsOrbPyramids of maxFrames slots and every intermediate array */
size_t ps_abi_sizeof_front_end_params(void);
/* Everything a frames call needs is allocated here -- maxFrames x max(1, maximalTrackedFeatures) rows of every intermediate
 * array and the detector's ROI lists -- so that call neither allocates nor waits.  pattern1024: HOST, NULL = the default.
 * Errors are those of ps_orb_detector_create and ps_orb_pyramids_create; maximalTrackedFeatures above PS_DBSCAN_MAX_KPTS ->
 * PS_ERR_UNSUPPORTED.  detect and describe are two cv::ORB objects in the reference (matcherOpenCV.cpp:66-67, :90) and may differ
 * here too: a descriptor with fewer levels drops the key points of the octaves it lacks.  Synchronous.  destroy waits for the
 * device; NULL is harmless. */
int ps_front_end_create(PsContext *ctx, int rows, int cols, int channels, const PsFrontEndParams *params, const int8_t *pattern1024,
                        int maxFrames, PsFrontEnd **out);
void ps_front_end_destroy(PsFrontEnd *fe);
/* Images and depth (DEVICE sets of the handle's shape, the same numFrames, at most maxFrames) in; desc F x capacity x 32 bytes,
 * out->pts and out->nkpts out: with maxKpts = capacity and strides 0 these three ARE a dense PsFrameSet for ps_vo_pairs_device.
 * The side arrays of `out` are those of ps_assemble_frames; its angleIn / responseIn / octaveIn are ignored (the handle's own key
 * points stand there).  capacity: at least what the detector can emit (as for ps_orb_detect_frames), at most max(1,
 * maximalTrackedFeatures) -- the rows the handle holds.  capacity above PS_DBSCAN_MAX_KPTS -> PS_ERR_UNSUPPORTED; a NULL, a shape
 * or stride that does not fit, numFrames that differ or exceed maxFrames, a capacity outside the range above -> PS_ERR_BAD_ARG
 * with a text in ps_last_error; outputs untouched.
 * numFrames == 0 is PS_OK.  Asynchronous on the context's stream. */
int ps_front_end_frames(PsContext *ctx, PsFrontEnd *fe, const PsImageSet *images, const PsDepthSet *depth, const PsFrameGeometry *geometry,
                        int capacity, uint8_t *desc, const PsFrameRowsOut *out);
/* The same for one frame: HOST pointers, uploads and downloads included, synchronous.  img rows x cols x channels bytes with
 * rowStride bytes between rows, depth rows x cols uint16 with depthStep bytes between rows (0 = dense either; a region keeps its
 * parent's -- the depth rule is the set's: what lies between the rows is not read).  desc cap x 32 bytes, out: HOST arrays of cap rows (pts required; nkpts ignored), *nout the rows.  Returns
 * PS_ERR_BAD_ARG with *nout = required capacity if cap is too small (nothing else is written); other errors as above. */
int ps_front_end_frame(PsContext *ctx, const uint8_t *img, const uint16_t *depth, int rows, int cols, int channels, size_t rowStride,
                       size_t depthStep, const PsFrontEndParams *params, const int8_t *pattern1024, const PsFrameGeometry *geometry,
                       uint8_t *desc, const PsFrameRowsOut *out, int cap, int *nout);

/* ---- Loop-closure candidates verified in one batch from the resident store: what the loop-closure thread does per candidate
 * (poseA, poseB) of FABMAP's priority queue -- FeaturesMap::loopClosure (src/Map/featuresMap.cpp:733-873) around
 * Matcher::matchFeatureLoopClosure (src/Matcher/matcher.cpp:802-861) -- for L candidates as two calls, no host step.
 *
 * ps_pose_sets_device inverts the store: for set s with q = poses[s], "the features observed from pose q, each with the
 * descriptor and the local 3-D point of THAT observation" (camTrajectory[q].featuresIds, a std::set<int>, featuresMap.cpp:785;
 * ExtendedDescriptor::descriptor / point3D, matcher.cpp:816-824).
 *   membership  feature f is a member iff one of its observations has obsPose == q; if a malformed store holds several such
 *               observations of one feature, the first (lowest observation index) is the one that is used;
 *   order       members appear in ascending feature index (the std::set's order);
 *   row         desc = that observation's 32 bytes, pts = the three (float) casts of its obsPoint3D, featIdx / obsIdx (when
 *               given) = the feature and the observation;
 *   counts      sets.nkpts[s] = setCount[s] = the count; sets.nkpts[S] = 0 is always written (the empty set: the verifier
 *               below parks gated candidates there);
 *   overflow    a count above maxKpts gives setCount[s] = -(count), nkpts[s] = 0, no row of that set is written, other sets
 *               are unaffected (the rule of viewCount / numMatches; call again with that capacity);
 *   bad pose    poses[s] outside 0 .. numPoses-1 gives setCount[s] = INT32_MIN, nkpts[s] = 0;
 *   bad range   THE RULE: if ANY feature of the store has an obsStart range that is not ascending inside 0 .. numObs
 *               (obsStart[f] < 0, obsStart[f+1] < obsStart[f] or obsStart[f+1] > numObs), every one of the S sets gets
 *               setCount = INT32_MIN, nkpts = 0 and no row is written -- a store whose index is broken is not read in part;
 *   other ids   an observation whose pose id lies outside 0 .. numPoses-1 belongs to no set (it is not an error);
 *   rows beyond the count are not written; the same pose may be listed twice, both sets are written.
 * The store's observation arrays are read twice (a count and an emit pass over the features, 256 a work-group) whatever S is:
 * a pose -> set table of numPoses ints, filled from `poses`, names the sets of each observation's pose.  No atomic decides an
 * order; the output does not depend on which work-group ran first.
 * S > PS_LOOP_MAX_SETS, maxKpts > PS_MAX_KPTS -> PS_ERR_UNSUPPORTED; a NULL array where one is needed, a negative count,
 * numFrames < S + 1, maxKpts < 1, bad strides (the rule of PsFrameSet), obsDesc not 16-byte aligned -> PS_ERR_BAD_ARG; outputs
 * untouched.  S == 0 writes nkpts[0] = 0 and returns PS_OK.  Asynchronous on the context's stream, copies nothing, does not
 * synchronise (growing scratch aside: 4 bytes per set and 256 features of the store, 4 bytes per pose). */
#define PS_LOOP_MAX_SETS 1024
typedef struct PsPoseSetRequest {     /* pointers: DEVICE */
    const double  *obsPoint3D;        /* O x 3: ExtendedDescriptor::point3D of each observation of the store (the feature in the
                                         observing pose's camera frame) -- the one array PsMapStore lacks */
    const int32_t *poses;             /* S pose ids */
    int32_t S, reserved;
} PsPoseSetRequest;
typedef struct PsPoseSetOut {         /* pointers: DEVICE, written by the call */
    PsFrameSet sets;                  /* numFrames >= S + 1, maxKpts <= PS_MAX_KPTS, dense or ABI-2 strides */
    int32_t *setCount;                /* S */
    int32_t *featIdx, *obsIdx;        /* numFrames x maxKpts each, or NULL */
} PsPoseSetOut;
int ps_pose_sets_device(PsContext *ctx, const PsMapStore *store, const PsPoseSetRequest *req, const PsPoseSetOut *out);

/* ps_loop_pairs_device: L candidates (pairs of SET indices) as one launch chain.
 *  1. gate: candidate l is RUN iff both set indices lie in 0 .. S-1, both setCount are >= 0, both are
 *     > minNumberOfFeaturesLC (strict, featuresMap.cpp:776-779) and both are >= 10 (matcher.cpp:830); otherwise its effective
 *     pair is (S, S), the empty set;
 *  2. the body of ps_vo_pairs_device on the effective pairs: params->errorVersion as given (the caller sets errorVersionMap,
 *     matcher.cpp:843-844), candidate l draws from cfg->seed + l, cfg->sampleIdx must be NULL;
 *  3. verdict: ratio[l] = 0.0 if gated (both reference gates leave 0), -1.0 if run and numMatches == 0 (:838-839), otherwise
 *     stats.pointInlierRatio (:859); closed[l] = ratio > matchingRatioThresholdLC (featuresMap.cpp:806; a NaN ratio is never
 *     closed); pairedRows[l] = (queryIdx, trainIdx) of the final inliers in match order (pairedFeatures, :853-857),
 *     numPaired[l] their count, pairedFeat[l] the two featIdx entries of each; empty lists for a gated or unmatched candidate.
 *     A candidate that names a set index outside 0 .. S-1 or a set with a negative count: numPaired = INT32_MIN, ratio = 0.0,
 *     closed = 0.
 * pair.* of a run candidate is byte for byte ps_match_hamming256 on the two sets followed by ps_ransac_rigid3d with seed + l;
 * of a gated one, what ps_vo_pairs_device gives for two empty frames.
 * NOTE: pairedRows are ROW indices into the two sets.  The reference's merge (featuresMap.cpp:824-856) compares these row
 * indices with feature IDS (featureB.id == pairFeat.second): it works only where rows and ids coincide.  Both forms are
 * returned; the merge itself (addMeasurements / removeFeatures) stays with the host, the store is replaced whole.
 * Argument rules are those of ps_vo_pairs_device: NULL where an array is needed (pairedFeat without featIdx included), L < 0,
 * S < 0, sets.numFrames < S + 1, bad strides -> PS_ERR_BAD_ARG; maxKpts > PS_MAX_KPTS -> PS_ERR_UNSUPPORTED; L == 0 is PS_OK. */
typedef struct PsLoopBatch {          /* pointers: DEVICE */
    PsFrameSet sets;                  /* as ps_pose_sets_device wrote them */
    const int32_t *setCount;          /* S */
    const int32_t *featIdx;           /* numFrames x maxKpts, or NULL */
    const int32_t *pairs;             /* L x 2 set indices: [0] = frameIds[0] (query / prev side), [1] = frameIds[1] */
    int32_t L, S;
    int32_t minNumberOfFeaturesLC;    /* featuresMap.cpp:776-779; shipped 35 */
    int32_t reserved;
    double matchingRatioThresholdLC;  /* :806; shipped 0.4 */
} PsLoopBatch;
typedef struct PsLoopResults {        /* pointers: DEVICE */
    PsPairResults pair;               /* L rows, row capacity sets.maxKpts */
    double  *ratio;                   /* L: what loopClosure logs as matchingRatio */
    int32_t *closed;                  /* L: ratio > matchingRatioThresholdLC */
    int32_t *numPaired;               /* L */
    int32_t *pairedRows;              /* L x maxKpts x 2: pairedFeatures (matcher.cpp:853-857) */
    int32_t *pairedFeat;              /* L x maxKpts x 2 feature indices of those rows, or NULL (needs featIdx) */
} PsLoopResults;
int ps_loop_pairs_device(PsContext *ctx, const PsRansacParams *params, const PsRansacConfig *cfg, const float *K,
                         const PsLoopBatch *batch, const PsLoopResults *out);
size_t ps_abi_sizeof_pose_set_request(void);
size_t ps_abi_sizeof_pose_set_out(void);
size_t ps_abi_sizeof_loop_batch(void);
size_t ps_abi_sizeof_loop_results(void);

/* ---- The resident store, its two inversions and the verifier for FLOAT descriptors (SURF / SIFT).  The reference runs the same
 * code for both descriptor kinds: matcher.cpp:675-679 copies whatever cv::Mat row the chosen observation holds,
 * matchFeatureLoopClosure (:802-861) pushes ext.descriptor rows into a Mat and calls performMatching, which for SURF / SIFT is
 * cv::BFMatcher(NORM_L2, true) (matcherOpenCV.cpp:100-102).  Everything that depends on the store's index arrays alone -- the
 * observation choice, steps 2 - 4, membership, order, counts -- is the binary calls' (the same kernels); what differs is the row.
 * A ROW IS COPIED AS 32-BIT WORDS, never through float arithmetic: NaN payloads, -0.0 and subnormals arrive bit for bit.  What
 * lies between the rows of a pitched output is never written.   */
typedef struct PsMapStoreF32 {    /* PsMapStore with float rows; DEVICE pointers */
    const double  *pos;           /* F x 3 */
    const int32_t *obsStart;      /* F + 1 */
    const int32_t *obsPose;       /* O */
    const float   *obsDesc;       /* O rows of dim floats, 4-byte aligned */
    const int32_t *obsOctave;     /* O */
    const double  *obsDetDist;    /* O */
    int32_t numFeatures, numObs, numPoses;
    int32_t dim;                  /* floats per row, 1 .. PS_MAX_L2_DIM */
    size_t obsDescRowStride;      /* bytes between rows: 0 = dense (dim x 4), else a multiple of 4 and >= dim x 4 */
} PsMapStoreF32;

typedef struct PsMapViewOutF32 {  /* PsMapViewOut with a float-descriptor set: drops into PsMapBatchF32::maps / mapLevel */
    PsFrameSetF32 views;          /* numFrames >= V, THE RULES of PsFrameSetF32 (pts is needed); views.dim == store.dim */
    int32_t *mapLevel;            /* numFrames x maxKpts */
    int32_t *viewCount;           /* V */
    int32_t *featIdx;             /* side arrays as in PsMapViewOut, each V x maxKpts rows or NULL */
    int32_t *obsIdx;
    double *posCam;
    double *uv;
    double *angle;
} PsMapViewOutF32;

/* ps_map_views_device for a PsMapStoreF32: the five steps, the count / overflow / INT32_MIN rules and the argument rules are that
 * call's, word for word, with PsMapViewRequest as it is; step 5's desc = the chosen observation's dim floats (matcher.cpp:675-679).
 * The rows are copied by a pass of their own after the emit kernel (ps_gather_rows_f32: one wavefront per row, consecutive
 * words), from the observation index of every row -- obsIdx, or a scratch block of 4 x V x maxKpts bytes when obsIdx is NULL.
 * No row of an overflowed or invalid view is written.
 * Beyond ps_map_views_device's errors: store.dim < 1, views.dim != store.dim, a row stride that is not a multiple of 4 or lies
 * below dim x 4, obsDesc not 4-byte aligned -> PS_ERR_BAD_ARG; dim > PS_MAX_L2_DIM -> PS_ERR_UNSUPPORTED; the output set follows
 * THE RULES of PsFrameSetF32.  Outputs untouched on any error; V == 0 is PS_OK. */
int ps_map_views_l2_device(PsContext *ctx, const PsMapStoreF32 *store, const PsMapViewRequest *req, const PsMapViewOutF32 *out);

typedef struct PsPoseSetOutF32 {      /* PsPoseSetOut with a float-descriptor set */
    PsFrameSetF32 sets;               /* numFrames >= S + 1, THE RULES of PsFrameSetF32 (pts is needed); sets.dim == store.dim */
    int32_t *setCount;                /* S */
    int32_t *featIdx, *obsIdx;        /* numFrames x maxKpts each, or NULL */
} PsPoseSetOutF32;

/* ps_pose_sets_device for a PsMapStoreF32: membership, order, counts, overflow, bad pose, bad range, "rows beyond the count are
 * not written", nkpts[S] = 0 and PS_LOOP_MAX_SETS are that call's, unchanged; a row's desc = that observation's dim floats
 * (matcher.cpp:816-818), copied by ps_gather_rows_f32 as above.  Errors as ps_pose_sets_device, with the store / set rules of
 * ps_map_views_l2_device in place of the 16-byte alignment of a binary store.  S == 0 writes nkpts[0] = 0. */
int ps_pose_sets_l2_device(PsContext *ctx, const PsMapStoreF32 *store, const PsPoseSetRequest *req, const PsPoseSetOutF32 *out);

typedef struct PsLoopBatchF32 {       /* PsLoopBatch with float-descriptor sets; pointers: DEVICE */
    PsFrameSetF32 sets;               /* as ps_pose_sets_l2_device wrote them */
    const int32_t *setCount;          /* S */
    const int32_t *featIdx;           /* numFrames x maxKpts, or NULL */
    const int32_t *pairs;             /* L x 2 set indices */
    int32_t L, S;
    int32_t minNumberOfFeaturesLC;
    int32_t reserved;
    double matchingRatioThresholdLC;
} PsLoopBatchF32;

/* ps_loop_pairs_device with the float matcher (matcherOpenCV.cpp:100-102,198-206) in place of the Hamming one: the same gate,
 * verdict, pairedRows / pairedFeat and invalid-candidate rules, PsLoopResults as it is.  pair.* of a run candidate is byte for
 * byte ps_match_l2_f32 on the two sets followed by ps_ransac_rigid3d with seed + l; of a gated one, what ps_vo_pairs_l2_device
 * gives for two empty frames.  The option "matcher_l2" changes no byte.  Argument rules as ps_loop_pairs_device, the sets under
 * THE RULES of PsFrameSetF32. */
int ps_loop_pairs_l2_device(PsContext *ctx, const PsRansacParams *params, const PsRansacConfig *cfg, const float *K,
                            const PsLoopBatchF32 *batch, const PsLoopResults *out);
size_t ps_abi_sizeof_map_store_f32(void);
size_t ps_abi_sizeof_map_view_out_f32(void);
size_t ps_abi_sizeof_pose_set_out_f32(void);
size_t ps_abi_sizeof_loop_batch_f32(void);

/* ---- A2, for a host that loops over batches (the loop of src/PUTSLAM/PUTSLAM.cpp:677-740 around Matcher::match,
 * src/Matcher/matcher.cpp:470-515): ps_vo_pairs_device through launch chains that are never joined.
 * One context is one launch chain: a batch's matrix-core Hamming sweep, then its vector scoring stages, dependent launches with
 * the chip partly idle between them.  A queue owns `chains` contexts + streams (0 = the default, 4; 1 .. PS_BATCH_QUEUE_MAX_CHAINS)
 * on ctx's device, with ctx's options, and hands batch n to chain n mod chains, WHOLE: consecutive batches run side by side, one
 * in its Hamming sweep while the others score -- 610 k instead of 517 k frame-pairs/s on batches of 499 pairs, 488 k instead of
 * 274 k at 125 pairs, 408 k instead of 142 k at 64 (round 6's measurements: splitting every batch over two chains, rounds 3 - 5's
 * recipe, gave 559 k at 499 pairs, profiles/r06h/queue_split_vs_turns.txt; FOUR chains are the best count at every batch size
 * from 16 to 1000 pairs, two read 601 k / 406 k / 183 k, six are worse than four: profiles/r06u/small_batch_chains.txt).  The chains'
 * contexts carry option "side_by_side" = chains: with other chains filling the gaps between its dependent launches the staged
 * scoring pays from 2 - 5 times smaller batches on than it does for a lone context (profiles/r06u/bench_data_crossover.txt).
 * The chains are ordered only within themselves; for a host that gives batches in flight output blocks of their own, nothing ever
 * makes one wait for another (the one exception is under submit: a block shared by batches in flight on several chains).
 *   submit: arguments of ps_vo_pairs_device (device pointers); pair p draws from cfg->seed + p: the outputs are byte for byte
 *           those of ONE ps_vo_pairs_device call.  Returns at once; *ticket (may be NULL) names the batch.  Inputs and outputs
 *           must stay valid until the batch is complete.  Batches in flight run CONCURRENTLY: give consecutive batches output
 *           blocks of their own (`chains` blocks used in turn are enough: batch n + chains runs on batch n's chain, behind it).
 *           A batch that is handed the block of batches still in flight is ordered behind them -- the block holds the results
 *           of the batch submitted last, row by row -- instead of racing them (csrc/ps_queue_hazard.h; every batch still in
 *           the ring is looked at, whatever else its chain has been given since):
 *             - the writers in flight all sit on one chain: the batch follows them on that chain, whole, whatever chain its
 *               number names and whether or not it would have been split -- correct, and as fast as one context; no chain waits;
 *             - they sit on several chains (a whole batch after a split one, PUTSLAM_HIP_QUEUE_SPLIT_FROM; split batches with
 *               different bounds): a whole batch runs on one of those chains, which waits (device-side, hipStreamWaitEvent) for the
 *               others' events; a split batch keeps its bounds and every share waits for the shares in flight on other chains
 *               whose rows it writes.  Split after split with the same bounds needs nothing: chain by chain they are in order.
 *             Only rows count: a shorter batch is not ordered behind shares that write rows it does not have.
 *           The block is identified by out->pose ALONE (a batch without a pose array: by NULL, all such batches as one block).
 *           Blocks with different pose arrays that share any other array (matches, numMatches, inlierMask, stats), and arrays
 *           that overlap without being equal, are not seen: keeping those apart stays the host's responsibility.
 *           Reading a batch's results needs its ticket waited for.  At most 64 batches are in flight: the 65th submit waits for
 *           the first.  If the chain's call fails the error is returned (text: ps_last_error of ctx); the ticket still stands
 *           for whatever part of the batch was queued.
 *   wait / query: the host blocks until / asks whether that batch is complete (query: 1 complete, 0 not yet).
 *   wait_on_stream: the given hipStream_t waits for the batch instead (device-side; the host does not block): what a host
 *           that post-processes on a stream of its own queues behind a batch.  A device-side wait for a batch that is still
 *           running is not free: while it is pending the chains themselves lose 5 % (499 pairs per batch) to 19 % (125) of
 *           their rate (profiles/r06v/pending_waits.txt) -- a host that can, queues its dependent work once query / wait says
 *           the batch is complete (the sharding layer and bench.py issue their gathers that way).
 *   context(q, i): chain i's context -- for ps_context_stream (work to be queued behind that chain's batch),
 *           ps_context_enable_timing, options; not for calls of its own while batches are in flight.
 *   last_split: bounds[0 .. chains] of the last submitted batch: pairs [bounds[i], bounds[i+1]) ran on chain i (all of them on
 *           one chain, unless PUTSLAM_HIP_QUEUE_SPLIT_FROM=<pairs> asks for rounds 3 - 5's split of batches that large: A/B runs).
 * Hardware queues: every chain wants one of its own.  The HIP runtime gives a process GPU_MAX_HW_QUEUES of them (default 4,
 * shared with the host's other streams) and serialises streams that share one.  The library sets GPU_MAX_HW_QUEUES=16 when it
 * is loaded if the variable is unset (a constructor, before the process' first HIP call for a program that links the library;
 * a host that set the variable keeps its value).  Read-only option "hw_queues_seen" = the value found; ps_batch_queue_create
 * leaves a warning in ps_last_error(ctx) when it is too small.  A process that initialises HIP before loading the library sets
 * the variable itself (putslam_amd/_lib.py does). */
#define PS_BATCH_QUEUE_MAX_CHAINS 8
typedef struct PsBatchQueue PsBatchQueue;
int ps_batch_queue_create(PsContext *ctx, int chains, PsBatchQueue **out);
void ps_batch_queue_destroy(PsBatchQueue *q);
int ps_batch_queue_submit(PsBatchQueue *q, const PsRansacParams *params, const PsRansacConfig *cfg, const float *K,
                          const PsFrameSet *frames, const int32_t *pairs, int P, const PsPairResults *out, int64_t *ticket);
int ps_batch_queue_wait(PsBatchQueue *q, int64_t ticket);
int ps_batch_queue_query(PsBatchQueue *q, int64_t ticket);
int ps_batch_queue_wait_on_stream(PsBatchQueue *q, int64_t ticket, void *hipStream);
int ps_batch_queue_synchronize(PsBatchQueue *q);
int ps_batch_queue_chains(const PsBatchQueue *q);
PsContext *ps_batch_queue_context(PsBatchQueue *q, int chain);
int ps_batch_queue_last_split(const PsBatchQueue *q, int32_t *bounds);

/* ---- The path's only exchange between GPUs: what travels to the rank that composes the trajectories -- the one
 * sequential step of the reference, VO pose composition with the 0.1 m gate, src/PUTSLAM/PUTSLAM.cpp:735-740 -- is a 72-byte record
 * per pair: pose[16] (column-major) + numInliers + numMatchesIn, as PS_RECORD_FLOATS floats.  ONE launch on hipStream (NULL: the
 * context's stream) packs `pairs` records from a batch's device-resident results: rows [0, valid) from pose / stats, rows
 * [valid, pairs) zero-filled (ranks of a gather send blocks of one size).  Queued behind a batch on the chain it ran on
 * (ps_batch_queue_context(q, chain)), it reads the block before that chain's next batch can overwrite it.  include/putslam_shard.h
 * and bench.py's multi-rank steps pack with it (torch's slice assignments were five launches on the chain). */
#define PS_RECORD_FLOATS 18
int ps_pack_records_device(PsContext *ctx, void *hipStream, const float *pose, const PsRansacStats *stats, int valid, int pairs,
                           float *records);

/* ---- A2, streaming form: Matcher::match (src/Matcher/matcher.cpp:452-516) with the previous frame's
 * descriptors and 3-D points resident in HBM (the prevDescriptors / prevFeatures3D state, matcher.h:379-384).
 * The first push only stores the frame (detectInitFeatures, matcher.cpp:17-64) and returns *nmatches = -1;
 * every later push matches previous (query) against the new frame (train), runs the estimator selected by
 * cfg on the surviving matches and makes the new frame the previous one (:506-513).
 * Hypothesis stream of every push = cfg->seed (the caller varies it per frame if wanted).
 * matches / inlierMask: capacity maxKpts; pose column-major 4x4; host pointers.
 * A push is launch-bound, so from the third push with unchanged params / estimator / numHypotheses / K on, the
 * copy-in -> four kernels -> copy-out sequence is replayed from a captured hipGraph (one per frame slot; frame,
 * row count and seed travel as data).  Results are identical; PUTSLAM_HIP_NO_GRAPH=1 keeps ordinary launches. */
typedef struct PsVoStream PsVoStream;
int ps_vo_stream_create(PsContext *ctx, int maxKpts, PsVoStream **out);
void ps_vo_stream_destroy(PsVoStream *s);
/* Forget the resident frame: the next push is a first frame again (Matcher::detectInitFeatures, matcher.cpp:17-64). */
int ps_vo_stream_reset(PsVoStream *s);
int ps_vo_stream_push(PsVoStream *s, const PsRansacParams *params, const PsRansacConfig *cfg, const float *K,
                      const uint8_t *desc, size_t descStep, const float *pts, int n,
                      PsDMatch *matches, int *nmatches, uint8_t *inlierMask, float *pose, PsRansacStats *stats);

/* ---- A2, PIPELINED streaming form (BASELINE configs[2]: "500 frames streamed through Matcher -> USAC -> Kabsch"):
 * the same call shape -- frames arrive on the host one after the other, each is matched against its predecessor
 * (src/Matcher/matcher.cpp:452-516, loop src/PUTSLAM/PUTSLAM.cpp:677-740) -- with the results returned with a LAG instead
 * of inside the push, so that uploads, kernels and downloads of consecutive frames overlap.  Frames are collected into
 * chunks of `chunkFrames`; a full chunk is uploaded on a copy stream into a ring of frames resident in HBM (the last
 * frame of the previous chunk is still there: no halo is sent twice), runs as ONE batched call (ps_vo_pairs_device's
 * launches) on one of `lanes` private contexts in turn (stream + scratch arena each, so that one chunk's Hamming sweep runs
 * beside another's scoring sweep; a lane's stream may hold further chunks queued behind the running one), and its results come
 * back in one download into pinned host memory.  chunkFrames = 1 is the
 * lowest-latency setting, 64..256 the throughput setting; ps_vo_stream_push stays the synchronous per-frame form.
 *
 * Hardware queues: every lane, the upload stream and the download stream want a hardware queue of their own; the HIP runtime
 * gives a process GPU_MAX_HW_QUEUES of them (default 4) and lets streams share beyond that, which serialises what shares.  The
 * library sets GPU_MAX_HW_QUEUES = 16 itself when it is loaded and the variable is unset (see PsBatchQueue above); with fewer than lanes + 6 the downloads
 * are queued on the lanes' own streams instead of a stream of their own (results identical, 10 - 20 % slower).
 *
 * Small chunks (chunkFrames <= 4; 1 is the reference's own call shape): a chunk of one to four frames is launch-bound, so every
 * place keeps a private copy of its frames (the previous frame is read again from its pinned staging slot: no ring, no copy
 * stream, no event pair) and its whole chunk is seven launches on the place's lane -- frames in by a copy kernel, kernels 1 - 4,
 * results out by a kernel --, with row counts, seed and frame addresses travelling as data: 25 - 28 k frames/s at 0.2 ms of lag from
 * one host thread, twice the synchronous push.  (PUTSLAM_HIP_STREAM_GRAPH=1 replays each place's chunk from ONE captured hipGraph
 * instead: measured slower on this runtime, profiles/r06h/mini_chunks.txt.)  Frames go through the library's pinned staging
 * areas in this form (88 KB per 2000-keypoint frame) unless they are pinned packed blocks handed to
 * ps_vo_stream_push_many_packed, which are read in place (untouched until the pair that has a frame as its PREVIOUS frame has been
 * popped); pop_many's pointers are a copy.  PUTSLAM_HIP_STREAM_MINI=0 keeps the ring form for such chunks (results identical).
 *
 * Pair k of the stream (frames k, k+1 counted from the last reset; frame k is the query = previous frame) draws its
 * hypotheses from the seeded stream cfg->seed + k: the results are byte for byte those of ONE ps_vo_pairs_device call
 * over the whole sequence with the same cfg, whatever the chunking.
 *
 * ps_vo_stream_configure_async: parameters of the pipelined form, fixed until the next configure (which drains).  chunkFrames
 *   1..1024 (0 = 128), lanes 2..8 (0 = by chunk size: 2 from 48 frames per chunk on, 3 below, 6 for chunks of one to four frames).
 *   cfg->sampleIdx must be NULL.  The lanes inherit the options of the stream's context.  Throughput grows with the chunk: 417 /
 *   504 / 550 k frame-pairs/s at 125 / 250 / 500 frames of 2000 keypoints per chunk (1.2 / 2.0 / 2.7 ms from push to results).
 * ps_vo_stream_push_async: ONE frame (host pointers, rows of descStep bytes) is copied into the pinned staging area of
 *   the chunk being collected; the chunk is submitted when it is full.  Returns at once.
 * ps_vo_stream_push_many: numFrames frames laid out like a PsFrameSet on the HOST (desc numFrames x maxKpts x 32 B,
 *   pts numFrames x maxKpts x 3 floats, nkpts numFrames) are submitted as chunks of at most chunkFrames.  If desc and pts
 *   are pinned host memory (ps_host_alloc, hipHostMalloc, hipHostRegister) the upload reads them in place -- they must
 *   stay untouched until the results of their frames have been popped; pageable memory is staged through pinned buffers.
 *   Frames staged by push_async before are submitted first, as a chunk of their own.
 * ps_vo_stream_flush: submits a partly filled chunk.
 * Flow control: a chunk needs a PLACE (a meta block, device and pinned result blocks, events); there are lanes + `ahead` of
 *   them (context option "stream_ahead", 0 .. 8, or -1 = by chunk size, the default: 1 from 96 frames per chunk on, 2 from 48,
 *   else six places in all; read by configure_async).  An accepted chunk is uploaded and
 *   launched at once, on the next lane in turn -- behind that lane's running chunk if it has one --, so a lane never waits for
 *   the host between chunks.  A place is busy from the launch of its chunk until pop_many has returned its results (the pinned
 *   block they lie in changes hands: the place goes on with a spare one while the caller reads).  push_async (at the first frame of a chunk) / push_many return
 *   PS_ERR_BUSY -- and take nothing -- when there is no place: pop first.  (Pinned frames handed to push_many are read in
 *   place: untouched until their results have been popped, as before.)
 * Errors other than PS_ERR_BUSY from push_async / push_many / flush / reset (an allocation or a HIP call failed while a chunk
 *   was being queued): whatever part of that chunk was queued is drained, the chunk's frames are DROPPED AS A UNIT -- for
 *   push_async: every frame collected in the partly filled chunk, the one just pushed included; for push_many: the failing chunk
 *   and the frames after it in the call (chunks before it are in flight and keep their numbering) -- and the stream goes on as
 *   after ps_vo_stream_reset: the next frame has no predecessor, its pair is number 0 of a new epoch (cfg->seed + 0).  No
 *   place is lost, nothing is in flight that pop would not return.  The reference's convention (no exceptions, fallback
 *   outputs, src/TransformEst/RANSAC.cpp:77-80,161-164) has no counterpart for a lost frame: the status code is the signal.
 * ps_vo_stream_pop_many: results of the oldest chunk in flight, as HOST pointers into that lane's pinned result block
 *   (valid until the next pop_many / pop / configure / destroy of this stream).  wait = 0: out->count = 0 if that chunk
 *   has not finished (or nothing is in flight); wait = 1: blocks until it has.
 * ps_vo_stream_pop: the same, one pair at a time, copied out (matches / inlierMask: capacity maxKpts; *nmatches = -1 and
 *   PS_OK when nothing is ready / in flight).  PS_RESULTS_INLIERS: *nmatches = number of inliers, matches = the inlier
 *   matches, inlierMask all ones; PS_RESULTS_POSES: *nmatches = 0, pose and stats only.
 * ps_vo_stream_reset on a pipelined stream: the next frame has no predecessor (Matcher::detectInitFeatures) and pair
 *   numbering restarts at 0; a partly filled chunk is submitted first (its place was reserved by its first frame); chunks in
 *   flight or waiting are unaffected and keep their numbering (`epoch` tells them apart). */
/* What a chunk's download carries (ps_vo_stream_set_result_mode, before ps_vo_stream_configure_async):
 *   PS_RESULTS_FULL     every cross-check match + the inlier mask + pose + stats (34 KB per 2000-keypoint pair);
 *   PS_RESULTS_INLIERS  what Matcher::match hands back (matcher.cpp:452-516: estimatedTransformation, inlierMatches): the
 *                       inlier matches of every pair in input order -- the first stats[i].numInliers entries of
 *                       matches[i * maxKpts ...] -- + pose + stats; inlierMask is NULL (12 KB per pair);
 *   PS_RESULTS_POSES    pose + stats only; matches and inlierMask are NULL (108 bytes per pair: a host that only composes
 *                       the trajectory, PUTSLAM.cpp:735-740).
 * numMatches is the number of cross-check matches in every mode.  Modes 1 and 2 are written by a kernel straight into the
 * lane's pinned block (no copy engine, no blit kernel beside the other lanes' launches). */
typedef enum PsStreamResults { PS_RESULTS_FULL = 0, PS_RESULTS_INLIERS = 1, PS_RESULTS_POSES = 2 } PsStreamResults;
/* How frames lie on the host and in the ring (ps_vo_stream_set_frame_layout, before ps_vo_stream_configure_async):
 *   PS_FRAMES_TWO_ARRAYS  descriptors and points in two arrays (push_many's form): two uploads per chunk;
 *   PS_FRAMES_PACKED      every frame is ONE block [maxKpts x 32 B descriptors][maxKpts x 12 B points] padded to
 *                         ps_vo_stream_packed_stride() bytes (maxKpts x 44 rounded up to 16; 88 000 at 2000 keypoints) -- what
 *                         a front end that detects, describes and back-projects a frame naturally fills, the reference's
 *                         prevDescriptors / prevFeatures3D state (include/putslam/Matcher/matcher.h:379-384) as one block --,
 *                         the ring in HBM has the same layout (PsFrameSet strides) and a chunk is ONE transfer: the link does
 *                         not idle between a descriptor and a point upload (+ 10 ... 15 % at chunks of 125).
 *                         ps_vo_stream_push_many_packed reads pinned frames in place (pageable ones are staged);
 *                         push_async / push_many still work on such a stream: they fill packed staging blocks on the host. */
typedef enum PsStreamFrames { PS_FRAMES_TWO_ARRAYS = 0, PS_FRAMES_PACKED = 1 } PsStreamFrames;

typedef struct PsHostPairResults {
    const PsDMatch *matches;      /* count x maxKpts (PS_RESULTS_INLIERS: the inlier matches first; PS_RESULTS_POSES: NULL) */
    const int32_t *numMatches;    /* count */
    const uint8_t *inlierMask;    /* count x maxKpts (NULL unless PS_RESULTS_FULL) */
    const float *pose;            /* count x 16, column-major */
    const PsRansacStats *stats;   /* count */
    int64_t firstPair;            /* number of the first pair of the block since the reset it belongs to */
    int32_t count;                /* pairs in this block; 0 = nothing ready */
    int32_t maxKpts;
    int32_t epoch;                /* resets of the stream before this block's frames */
    int32_t resultMode;           /* PsStreamResults the block was written with */
} PsHostPairResults;
int ps_vo_stream_set_result_mode(PsVoStream *s, int mode /* PsStreamResults; takes effect at the next configure_async */);
int ps_vo_stream_configure_async(PsVoStream *s, const PsRansacParams *params, const PsRansacConfig *cfg, const float *K,
                                 int chunkFrames, int lanes);
int ps_vo_stream_push_async(PsVoStream *s, const uint8_t *desc, size_t descStep, const float *pts, int n);
int ps_vo_stream_push_many(PsVoStream *s, const uint8_t *desc, const float *pts, const int32_t *nkpts, int numFrames);
int ps_vo_stream_set_frame_layout(PsVoStream *s, int layout /* PsStreamFrames; takes effect at the next configure_async */);
size_t ps_vo_stream_packed_stride(const PsVoStream *s);
int ps_vo_stream_push_many_packed(PsVoStream *s, const uint8_t *frames, size_t frameStride, const int32_t *nkpts, int numFrames);
int ps_vo_stream_flush(PsVoStream *s);
int ps_vo_stream_pop_many(PsVoStream *s, int wait, PsHostPairResults *out);
int ps_vo_stream_pop(PsVoStream *s, int wait, PsDMatch *matches, int *nmatches, uint8_t *inlierMask, float *pose,
                     PsRansacStats *stats);
/* Pairs submitted or staged whose results have not been popped yet (negative PsStatus on error). */
int ps_vo_stream_pending(const PsVoStream *s);
/* Pushes (synchronous form) / chunks (pipelined form, chunkFrames <= 4) replayed from a captured hipGraph so far. */
long long ps_vo_stream_graph_launches(const PsVoStream *s);
/* Pinned (page-locked) host memory for frames handed to ps_vo_stream_push_many in place; NULL on failure. */
void *ps_host_alloc(size_t bytes);
void ps_host_free(void *p);

/* Algorithmic bytes one call of ps_vo_pairs_device moves per SURVEY.md section 8(d):
 * computed from the per-pair stats already on the host (numMatchesIn, numMatchesValid). */
uint64_t ps_algorithmic_bytes(int nkpts, int matchesIn, int matchesValid, int numHypotheses);

/* Names of the kernels launched by ps_vo_pairs_device, in launch order, NUL separated,
 * double-NUL terminated (used by the bench to pick rows out of rocprofv3 output). */
const char *ps_kernel_names(void);

/* Kernel timing: when enabled, every ps_vo_pairs_device call brackets each of its kernel
 * launches with HIP events recorded on the context's stream (the stream the kernels run on).
 * Enabling (again) resets the record; the last 128 calls are kept.
 * ps_last_kernel_times_ms: the most recent call (ms holds 8 floats; returns the kernel count).
 * ps_kernel_time_totals: sums and launch counts over all kept calls (arrays of 8). */
int ps_context_enable_timing(PsContext *ctx, int enable);
int ps_last_kernel_times_ms(PsContext *ctx, float *ms);
int ps_kernel_time_totals(PsContext *ctx, double *sum_ms, int *launches);

/* ---- diagnostics (used by the parity tests; no reference counterpart) -------------------- */
/* ps_ransac_rigid3d's scoring stage only: counts[h] = inlier count kernel 3 produced for
 * hypothesis h (0 for an invalid model); *numScored = hypotheses scored (<= cfg->numHypotheses:
 * the RANSAC estimator never needs more than max(iterations(0.2), iterations(minRatio))). */
int ps_debug_ransac_counts(PsContext *ctx, const PsRansacParams *params, const PsRansacConfig *cfg,
                           const float *K, const float *prev, int nprev, const float *cur, int ncur,
                           const PsDMatch *matches, int m, int32_t *counts, int *numScored);
/* Words of the context's keys block that are not all-ones once its queued work has drained; must be 0 after any sequence of
 * calls (the matcher's query splits merge with atomicMin on a block kernel 2 leaves all-ones: no clearing launch per call). */
int ps_debug_keys_clean(PsContext *ctx, uint64_t *bad);
/* Device-side trip limit after a best model with c inliers out of M, for c = 1..M:
 * min(H, iterations(minRatio), iterations(float(c)/float(M))) for PS_EST_RANSAC (RANSAC.cpp:450-461),
 * min(H, updateStandardStopping(c, M, 3)) for PS_EST_USAC (USAC.h:944-971). */
int ps_debug_limits(PsContext *ctx, int estimator, double minRatio, int H, int M, int32_t *out);
/* Runs blocks*256*perThread random (a0, a1, b) triples through the scoring kernel's shared-reciprocal
 * division and through the '/' operator; *mismatches must come back 0 (bitwise comparison). */
int ps_debug_fastdiv(PsContext *ctx, uint64_t seed, int blocks, int perThread, uint64_t *mismatches, uint64_t *tested);
/* The exact short forms of sqrt / reciprocal / shared-denominator quotients inside the hypothesis prologue (the float
 * Umeyama + Jacobi SVD of RANSAC.cpp:207-244 and the 4x4 inverse of :337-338) against sqrtf and '/', bit for bit; *mismatches
 * must come back 0.  mode 0: every float from 1.0f to +inf and beyond (elements = 0x40001000), 1: every float of [1, 2]
 * (0x00800001), 2: y / |y|, 3: 1 / d and u / d with d = sqrt(1 + u u), 4: nine numerators over one denominator (random). */
int ps_debug_mathcheck(PsContext *ctx, int mode, uint64_t seed, uint64_t elements, uint64_t *mismatches, uint64_t *tested);
/* After a scoring launch with option "score_stats" = 1: evaluations the fast kernel parked for the value-exact
 * code, and (hypothesis, match) evaluations it made in all (lanes of partially filled wavefronts included). */
int ps_debug_score_stats(PsContext *ctx, uint64_t *parked, uint64_t *evaluations);
/* All eight counters of the last scoring step: [0] parked, [1] evaluations made (with the staged scoring: what is left of
 * the complete sweep of H hypotheses x M matches); [2] / [3] trips (wavefront x two matches) of stage 1's pre-test that left
 * no lane / some lane to the value-exact test; [4..7] reserved (0). */
int ps_debug_score_stats_ex(PsContext *ctx, uint64_t *out8);
/* Staged scoring: hypotheses of every pair that survived stage 1 (out[0..P)) and stage 2 (out[P..2P)) of the last call
 * that was scored in stages: zeros if the LAST scoring step of the context was not staged, PS_ERR_BAD_ARG if P is not that
 * step's number of pairs (the counters are laid out with it; option "last_staged_pairs" says how many pairs that was). */
int ps_debug_stage_survivors(PsContext *ctx, int P, int32_t *out);
/* Staged scoring with the reordered match record: perm[P][cap] = for every pair, the match (index into its depth-valid
 * matches) at each position of the order stages 1+ swept; front[P] = leading positions whose matches every voting hypothesis
 * rejected and found far off (stage 1's pre-test range).  Entries beyond a pair's number of valid matches are unspecified.
 * PS_ERR_BAD_ARG unless the context's last scoring step was staged AND reordered with exactly this P and cap. */
int ps_debug_stage_order(PsContext *ctx, int P, int cap, int32_t *perm, int32_t *front);
/* Latency study (option "stamps" = 1): the shader-clock stamps (s_memtime) work-group 0 of kernels 2 and 4 of the last call
 * wrote into a private buffer: out16[0..3] = ps_crosscheck_prep (start, best[q] built, matches compacted + records written,
 * end), out16[4..9] = ps_select_refit (start, selection replayed, winner's inlier pass, refit, re-selection, end). */
int ps_debug_stamps(PsContext *ctx, uint64_t *out16);
/* Diagnostic of the float matcher's matrix-core prefilter (option "matcher_l2" = 1, dim 64 / 128): for
 * one pair of host arrays as ps_match_l2_f32 takes them, the prefilter's estimate s~(t, q) of the squared distance and its band
 * E(t, q), as two nt x nq row-major float arrays (train row major).  The band's claim: |s~ - S| <= E and |L2sqr - S| <= E for
 * the real-number S.  dim other than 64 / 128 -> PS_ERR_UNSUPPORTED. */
int ps_debug_l2_band(PsContext *ctx, const float *query, int nq, size_t qstepBytes, const float *train, int nt, size_t tstepBytes,
                     int dim, float *stilde, float *band);
/* Diagnostic counters of the last float matching call that ran the prefilter while option "l2_stats" was 1: out3 = {train rows
 * swept exactly, candidate (t, q) evaluations of the other rows, rows whose candidate list overflowed}. */
int ps_debug_l2_stats(PsContext *ctx, uint64_t *out3);
/* DBScan's neighbour predicate in the square domain: the least double s* with (double)(float)sqrt(s*) >= eps (0 for eps <= 0
 * or NaN), so that (float)sqrt(s) < eps  <=>  s < s*.  Pure host arithmetic. */
double ps_debug_dbscan_bound(double eps);
/* sizeof() of the PODs as compiled into the library (layout check for foreign-language bindings). */
size_t ps_abi_sizeof_dmatch(void);
size_t ps_abi_sizeof_params(void);
size_t ps_abi_sizeof_config(void);
size_t ps_abi_sizeof_stats(void);
size_t ps_abi_sizeof_frameset(void);
size_t ps_abi_sizeof_results(void);
size_t ps_abi_sizeof_host_results(void);
size_t ps_abi_sizeof_map_batch(void);

/* ---- The tracking VO step (VOVersion = 1): Matcher::trackKLT, src/Matcher/matcher.cpp:147-211, for P pairs with no host step
 * -- track, select, undistort and back-project the tracked positions, carry the key points' columns along, and run the estimator
 * on the DMatch(i, j, 0) lists the selection wrote.  Three calls: the estimator over caller-supplied device-resident match lists,
 * the tracked rows, and the whole step.  DESIGN.md section 8.14. */
typedef struct PsPointSets {  /* numSets blocks of 3-D points, DEVICE */
    const float *pts;        /* set s: capacity x 3 floats from pts + s x setStride bytes */
    const int32_t *counts;   /* numSets: the rows of every set that are points */
    int32_t numSets, capacity;
    size_t setStride;        /* BYTES between sets, 0 = dense (capacity x 12); a multiple of 4, at least capacity x 12 */
} PsPointSets;
size_t ps_abi_sizeof_point_sets(void);

/* RANSAC::estimateTransformation (RANSAC.cpp:50-174) / RANSAC_USAC (USAC_wrapper.cpp:104-151) for P pairs with the caller's match
 * lists.  Pair p matches set pairs[2p] of `prev` (queryIdx) with set pairs[2p + 1] of `cur` (trainIdx); pairs = NULL: set p of
 * both.  matches P x cap, numMatches P, pairs P x 2 int32: DEVICE, as is everything `prev`, `cur` and `out` point to.  out:
 * inlierMask P x cap, pose P x 16, stats P; its matches / numMatches are ignored and may be NULL.  cfg->sampleIdx must be NULL;
 * pair p draws from cfg->seed + p.  Asynchronous on the context's stream; only the context's scratch may grow.
 * For every pair the mask, the pose and the statistics are, byte for byte, those of ps_ransac_rigid3d on (prev set, cur set,
 * matches[p], numMatches[p]) with seed cfg->seed + p.  What that host form refuses, and device data may still hold, is decided
 * here:
 *  - a match whose queryIdx / trainIdx lies outside 0 .. count-1 of its set is never followed: it is dropped like a match that
 *    fails the depth gate (RANSAC.cpp:65-74), its mask byte is 0, and pointInlierRatio does not count its trainIdx.  The results
 *    are those of the list without it, except that stats.numMatchesIn stays numMatches[p] and the mask keeps the list's positions;
 *  - numMatches[p] outside 0 .. cap, a pair index outside its group of sets, or a set count outside 0 .. capacity: the list counts
 *    as empty -- identity pose, NO mask byte written, the statistics of a list below minimalNumberOfMatches (RANSAC.cpp:77-80)
 *    with numMatchesIn = 0.
 * NULL params / cfg / prev / cur / out or (P > 0) a NULL array, P < 0, cap < 1, cap above 1 << 22, a set stride that breaks the rule
 * above, a sampleIdx -> PS_ERR_BAD_ARG; capacity of `cur` above PS_MAX_KPTS -> PS_ERR_UNSUPPORTED; text in ps_last_error.  P == 0 is PS_OK. */
int ps_ransac_match_lists(PsContext *ctx, const PsRansacParams *params, const PsRansacConfig *cfg, const float *K,
                          const PsPointSets *prev, const PsPointSets *cur, const int32_t *pairs, const PsDMatch *matches,
                          const int32_t *numMatches, int P, int cap, const PsPairResults *out);

typedef struct PsTrackedCarry {  /* the previous rows' key point columns, DEVICE, P x capacity each; NULL = not carried */
    const float *angle, *response;
    const int32_t *octave;
    const double *detDist;   /* prevDetDists: carried, not recomputed (matcher.cpp:183-186) */
} PsTrackedCarry;
typedef struct PsTrackedRows {   /* the rows a tracked frame leaves, DEVICE, P x capacity rows each (counts: P) */
    float *xy;               /* x 2: the tracked (distorted) position -- prevFeaturesDistorted of the next frame; required */
    float *xyUndist;         /* x 2; NULL = not wanted */
    float *pts;              /* x 3: features3D; required */
    int32_t *counts;         /* required */
    float *angle, *response; /* each wanted exactly where its PsTrackedCarry column is given: both or neither */
    int32_t *octave;
    double *detDist;
} PsTrackedRows;
size_t ps_abi_sizeof_tracked_carry(void);
size_t ps_abi_sizeof_tracked_rows(void);

/* The tracked rows, matcher.cpp:159-186, for P pairs.  For output row j < numKept[p] with i = keptIdx[p][j]: out->xy[p][j] =
 * nextPts[p][i]; xyUndist = the arithmetic of ps_remove_image_distortion on it; pts = the arithmetic of ps_keypoints2Dto3D on
 * xyUndist in depth frame depthFrame[p] under ps_assemble_frames' rule (the frame alone, as the DENSE image the reference holds);
 * angle / response / octave / detDist [p][j] = carry's [p][i].  out->counts[p] = numKept[p]; where that lies outside 0 ..
 * capacity (the -1 of ps_klt_select_device) counts[p] = -1 and nothing else is written for the pair.  An index outside 0 ..
 * capacity-1 is not followed: the row is written as zeros.  A depthFrame[p] outside 0 .. numFrames-1 gives points of depth 0, the
 * keypoints2Dto3D result for no depth.  Nothing is written beyond a pair's count.  nextPts P x capacity x 2 floats, keptIdx P x
 * capacity, numKept and depthFrame P int32: DEVICE.  carry may be NULL (nothing carried).  THE ROWS OF ONE FRAME ARE THE PREVIOUS
 * ROWS OF THE NEXT: xy / pts / counts / the carried columns, unchanged, are what ps_track_vo_pairs takes as prevXY / prevPts /
 * prevCounts / prev.  A NULL among geometry, depth, depthFrame, nextPts, keptIdx, numKept, out, out->xy, out->pts, out->counts, a
 * carried column without its output or the reverse, a depth set whose strides do not resolve or (P > 0) without pixels, capacity
 * < 1, P outside 0 .. 65535 -> PS_ERR_BAD_ARG; capacity above PS_MAX_KPTS -> PS_ERR_UNSUPPORTED; P == 0 is PS_OK.  One launch,
 * asynchronous; no scratch.
 * THE OUTPUT BLOCKS MUST NOT OVERLAP THE INPUTS: a row is read at keptIdx[p][j] while other rows are written at j, so rows cannot be
 * assembled in place -- a chain alternates between two sets of blocks (device_batch.run_tracked_sequences allocates one per step). */
int ps_assemble_tracked(PsContext *ctx, const PsFrameGeometry *geometry, const PsDepthSet *depth, const int32_t *depthFrame,
                        const float *nextPts, const int32_t *keptIdx, const int32_t *numKept, int P, int capacity,
                        const PsTrackedCarry *carry, const PsTrackedRows *out);

typedef struct PsTrackVoParams {
    double trackingErrorThreshold;                   /* OpenCVParams.trackingErrorThreshold */
    double minimalReprojDistanceNewTrackingFeatures; /* OpenCVParams.minimalReprojDistanceNewTrackingFeatures */
    int32_t removeTooCloseFeatures;                  /* must be 0 (below) */
    int32_t reserved;
} PsTrackVoParams;
typedef struct PsTrackVoIn {     /* DEVICE pointers */
    const int32_t *pairs;        /* P x 2: (previous, current) slots of the pyramid set */
    const int32_t *depthFrame;   /* P: the depth frame of every pair; NULL = the pair's current slot */
    const float *prevXY;         /* P x capacity x 2: prevFeaturesDistorted */
    const float *prevPts;        /* P x capacity x 3: prevFeatures3D */
    const int32_t *prevCounts;   /* P */
    PsTrackedCarry prev;         /* prevKeyPoints' columns and prevDetDists */
} PsTrackVoIn;
typedef struct PsTrackVoOut {    /* DEVICE pointers, P x capacity rows each unless noted */
    float *nextPts;              /* x 2; the tracker's: caller-owned intermediates, all three required; nextPts is READ under */
    uint8_t *status;             /*      PS_KLT_USE_INITIAL_FLOW, as for ps_klt_track_device */
    float *err;
    PsDMatch *matches;           /* DMatch(i, j, 0): ps_klt_select_device's; required with numMatches and keptIdx */
    int32_t *numMatches;         /* P */
    int32_t *keptIdx;
    PsTrackedRows rows;          /* the frame's rows: ps_assemble_tracked's; rows.xy is also the selection's keptPts */
    uint8_t *inlierMask;         /* over matches; required with pose and stats */
    float *pose;                 /* P x 16 column-major */
    PsRansacStats *stats;        /* P */
} PsTrackVoOut;
size_t ps_abi_sizeof_track_vo_params(void);
size_t ps_abi_sizeof_track_vo_in(void);
size_t ps_abi_sizeof_track_vo_out(void);

/* matcher.cpp:147-211 for P pairs of slots of a pyramid set, as one queue of launches on the context's stream: the launch of
 * ps_klt_track_device on (in->pairs, in->prevXY, in->prevCounts), the launch of ps_klt_select_device with tp's two thresholds,
 * the launch of ps_assemble_tracked, and the chain of ps_ransac_match_lists on (in->prevPts with prevCounts, out->rows.pts with
 * rows.counts, out->matches) with pair p = (set p, set p) and params->errorVersion as given (the caller puts errorVersionVO
 * there).  It neither waits nor downloads; only the context's RANSAC scratch may grow.  A pair with prevCounts[p] == 0 gives the
 * identity and no matches (:147-148); a pair whose count the selection refuses (-1) gives rows.counts[p] = -1 and the results of
 * an empty list.  The rows of a call, unchanged, are the previous rows of the next (ps_assemble_tracked): a tracked sequence
 * chains on one stream until a refill is due.
 * tp->removeTooCloseFeatures != 0 -> PS_ERR_UNSUPPORTED: the reference erases the removed features from features3D and leaves the
 * surviving matches' trainIdx un-renumbered (matcher.cpp:960-963), so that RANSAC reads features3D at stale indices, possibly
 * beyond its end -- there is no defined behaviour to restate; the shipped value is 0 (putslammatcherOpenCVParameters.xml:77), and
 * a host that wants the filter runs ps_exclude_device itself.  Other errors are those of the four calls, all found before the first
 * launch; outputs untouched.  No block of `out` may overlap a block of `in` (ps_assemble_tracked's rule: the next call takes this
 * call's rows as its previous rows and writes OTHER blocks). */
int ps_track_vo_pairs(PsContext *ctx, const PsKltPyramids *pyr, const PsKltParams *klt, const PsTrackVoParams *tp,
                      const PsRansacParams *params, const PsRansacConfig *cfg, const PsFrameGeometry *geometry, const PsDepthSet *depth,
                      const PsTrackVoIn *in, int P, int capacity, const PsTrackVoOut *out);

/* The same for one pair: HOST pointers, uploads and downloads included, synchronous.  prevImg / nextImg rows x cols x channels bytes
 * with rowStride bytes between rows, depth (the current frame's) rows x cols uint16 with depthStep bytes between rows (0 = dense
 * either; a region keeps its parent's -- the depth rule is the set's: what lies between the rows is not read).  in: prevXY n x 2,
 * prevPts n x 3 and the carried columns of n rows (pairs, depthFrame and prevCounts are ignored); out: HOST arrays of n rows --
 * nextPts, matches, keptIdx, inlierMask, pose (16) and stats (1) required, the others NULL = not wanted; nextPts is read under
 * PS_KLT_USE_INITIAL_FLOW; a carried column is returned only where `in` has it.  *numKept = the rows kept (also written to
 * out->numMatches and out->rows.counts where given); the tracker's arrays are written for all n points, the others for the kept
 * rows.  n == 0 gives the identity and the statistics of the empty list.  n above PS_MAX_KPTS -> PS_ERR_UNSUPPORTED; other errors
 * as above and as ps_perform_tracking's. */
int ps_track_vo_pair(PsContext *ctx, const uint8_t *prevImg, const uint8_t *nextImg, const uint16_t *depth, int rows, int cols, int channels,
                     size_t rowStride, size_t depthStep, const PsKltParams *klt, const PsTrackVoParams *tp, const PsRansacParams *params,
                     const PsRansacConfig *cfg, const PsFrameGeometry *geometry, const PsTrackVoIn *in, int n, const PsTrackVoOut *out,
                     int *numKept);

/* ---- Closing the tracking VO step: Matcher::trackKLT, src/Matcher/matcher.cpp:213-381 -- the refill when fewer than
 * minimalTrackedFeatures rows survive (:213-279), the predicted pyramid level of every row (:281-301), the stable reordering by
 * that level (:302-331), describeFeatures at the predicted level (:338) and the removal of the rows the descriptor extractor
 * dropped (:343-381) -- for P pairs with no host step.  DESIGN.md section 8.15. */
typedef struct PsTrackCandidates {  /* the sandbox of :218-246 for numFrames frames, DEVICE, numFrames x capacity rows each */
    const float *xy, *xyUndist;  /* x 2 */
    const float *pts;            /* x 3 */
    const float *angle, *response;
    const int32_t *octave;
    const double *detDist;
    const int32_t *counts;       /* numFrames */
    int32_t numFrames, capacity; /* capacity 1 .. PS_EXCL_MAX_CAND */
} PsTrackCandidates;
typedef struct PsTrackCloseParams {
    double minimalReprojDistanceNewTrackingFeatures; /* OpenCVParams.minimalReprojDistanceNewTrackingFeatures */
    int32_t minimalTrackedFeatures;                  /* OpenCVParams.minimalTrackedFeatures */
    int32_t removeTooCloseFeatures;                  /* must be 0, as for ps_track_vo_pairs (:274-277 is the same case) */
} PsTrackCloseParams;
typedef struct PsTrackCloseOut {    /* DEVICE, P x outCapacity rows each unless noted */
    uint8_t *desc;               /* x 32 bytes: with rows.pts and rows.counts a dense PsFrameSet of maxKpts = outCapacity */
    PsTrackedRows rows;          /* every column required; octave is the DETECTION octave (keyPoints, not descKeyPoints) */
    int32_t *srcIdx;             /* the tracked row the output row was, or capacity + i for candidate i */
    int32_t *refill;             /* P: 0 = not due, 1 = the candidates were merged, 2 = due but no candidates were given */
} PsTrackCloseOut;
typedef struct PsTrackClose PsTrackClose; /* every intermediate array of ps_track_close_pairs: merged rows, levels, keptIdx */
size_t ps_abi_sizeof_track_candidates(void);
size_t ps_abi_sizeof_track_close_params(void);
size_t ps_abi_sizeof_track_close_out(void);

/* The sandbox for every frame of a device-resident set, on a PsFrontEnd's detector and arrays: ps_orb_detect_frames,
 * ps_dbscan_thin_device (minPts 2, featuresFromCluster 1) and ps_assemble_frames on DBScan's keptIdx with every side column --
 * out->xy, xyUndist, pts, angle, response, octave, detDist and nkpts are all required (srcIdx optional, angleIn / responseIn /
 * octaveIn ignored); nothing is described.  With counts = out->nkpts these are a PsTrackCandidates.  images, depth, geometry and
 * capacity as for ps_front_end_frames, errors as there; outputs untouched.  Only the ORB detector has a handle of this layout: a
 * FAST sandbox is not offered.  Asynchronous on the context's stream. */
int ps_track_candidates(PsContext *ctx, PsFrontEnd *fe, const PsImageSet *images, const PsDepthSet *depth, const PsFrameGeometry *geometry,
                        int capacity, const PsFrameRowsOut *out);

/* Room for calls of up to maxPairs pairs x maxRows rows (maxPairs 1 .. 65535, maxRows 1 .. PS_MAX_KPTS), allocated here so that a
 * call neither allocates nor waits.  Synchronous.  destroy waits for the device; NULL is harmless. */
int ps_track_close_create(PsContext *ctx, int maxPairs, int maxRows, PsTrackClose **out);
void ps_track_close_destroy(PsTrackClose *tc);

/* matcher.cpp:213-381 for P pairs.  tracked: the rows a ps_track_vo_pairs call left, P x capacity, EVERY column (xy, xyUndist,
 * pts, counts, angle, response, octave, detDist) required -- the level rule needs octave and detDist, the merge xyUndist.  cand:
 * candidate rows (ps_track_candidates') or NULL; candFrame[p] names the frame of `cand` that is pair p's sandbox, a value outside
 * 0 .. cand->numFrames-1 (-1) or cand == NULL (candFrame may then be NULL too) means none.  pyr: ORB pyramids the caller has
 * built (ps_orb_pyramids_build_device); pair p is described in slot slots[p], and pairs that look at one image name one slot --
 * one build serves all pairs.  Four launches on the context's stream:
 *  1. per pair, n = tracked->counts[p]: the refill is DUE iff n < tp->minimalTrackedFeatures, evaluated on the device.  A due pair
 *     with candidates runs mergeTrackedFeatures (:97-130): candidate i, in ascending index, is appended behind the tracked rows iff
 *     no tracked row and no PREVIOUSLY APPENDED candidate is near it -- (double)du * du + (double)dv * dv <
 *     ps_sqrt_bound_f64(minimalReprojDistanceNewTrackingFeatures) on the float differences of the undistorted positions (the
 *     predicate of ps_exclusion_rule_merge_tracked; false with a NaN).  Candidates of a pair that is not due are ignored.  Then
 *     every merged row's predicted level: curDist = the float root of ((x * x + y * y) + z * z) in floats (:287-290 as compiled:
 *     ps_assemble_frames' detDist arithmetic), level = THE LEVEL RULE above on (octave, detDist, curDist) -- scaleFactor 1.2,
 *     nLevels 8 (matcher.h:26-28); a quotient that is not finite (curDist 0) gives level 0; an octave outside
 *     PS_LEVEL_OCTAVE_MIN .. MAX gives level -1, and the description then drops the row (an extension: the reference has no such
 *     key point).
 *  2. + 3. ps_describe_features_device's two launches on the merged xy, angle and the LEVEL as octave: its stable grouping by
 *     octave is :302-331, its border rule (31 <= x < cols - 31, 31 <= y < rows - 31) the "unlucky case" of :343-381 -- the
 *     position-matching walk of :359-375 selects exactly its keptIdx, the border test depending on the position alone.  A level
 *     the pyramid set lacks drops the row.  out->desc receives the rows.
 *  4. every column gathered by keptIdx into out->rows, out->srcIdx, out->rows.counts[p].
 * out->refill[p]: 0 not due, 1 merged, 2 due with no candidates -- the rows are then closed without the refill, a departure the
 * flag reports.  A tracked count outside 0 .. capacity, or (on a due pair with candidates) a candidate count outside 0 ..
 * cand->capacity, gives out->rows.counts[p] = -1 and nothing else is written for the pair, refill[p] included.  Nothing is written beyond a pair's
 * count.  outCapacity >= capacity + cand->capacity (0 without cand), at most the handle's maxRows; P at most its maxPairs.
 * The closed rows, unchanged, are prevXY / prevPts / prevCounts / prev of the next ps_track_vo_pairs (capacity = outCapacity).
 * tp->removeTooCloseFeatures != 0 -> PS_ERR_UNSUPPORTED (ps_track_vo_pairs' reason).  NULL where an argument or array is needed,
 * a tracked or output column absent, P < 0 or above maxPairs, capacity < 1, outCapacity outside the range above, a cand with
 * numFrames < 1 or a NULL column -> PS_ERR_BAD_ARG; outCapacity above PS_MAX_KPTS or cand->capacity above PS_EXCL_MAX_CAND ->
 * PS_ERR_UNSUPPORTED.  Everything that can refuse the call is found before the first launch: outputs untouched.  P == 0 is PS_OK.
 * Outputs must not overlap inputs.  Asynchronous; the call neither allocates nor waits (the level rule's table is uploaded at a
 * context's first use of it, as for ps_frame_levels_device). */
int ps_track_close_pairs(PsContext *ctx, PsTrackClose *tc, const PsOrbPyramids *pyr, const int32_t *slots, const PsTrackCloseParams *tp,
                         const PsTrackedRows *tracked, const PsTrackCandidates *cand, const int32_t *candFrame, int P, int capacity,
                         int outCapacity, const PsTrackCloseOut *out);

/* The same for one pair: HOST pointers, uploads and downloads included, synchronous.  img rows x cols x channels bytes with
 * rowStride bytes between rows, depth (the same frame's) rows x cols uint16 with depthStep bytes between rows (0 = dense either; a
 * region keeps its parent's).  params: the detector of the sandbox and the descriptor's pyramid (PsFrontEndParams; pattern1024 as
 * for ps_front_end_create); tracked: HOST arrays of n rows, every column (counts is ignored).  The pyramid is built here; the
 * sandbox (ps_track_candidates) runs only when the refill is due, n < tp->minimalTrackedFeatures.  desc cap x 32 bytes, out: HOST
 * arrays of cap rows (NULL = not wanted; counts, if given, receives the rows), srcIdx cap int32 -- a candidate's is max(n, 1) + i --,
 * *nout the rows, *refill the flag.  Returns PS_ERR_BAD_ARG with *nout = required capacity if cap is too small (nothing else is
 * written but *refill); n above PS_MAX_KPTS -> PS_ERR_UNSUPPORTED; other errors as above and as ps_front_end_create's. */
int ps_track_close_pair(PsContext *ctx, const uint8_t *img, const uint16_t *depth, int rows, int cols, int channels, size_t rowStride,
                        size_t depthStep, const PsFrontEndParams *params, const int8_t *pattern1024, const PsFrameGeometry *geometry,
                        const PsTrackCloseParams *tp, const PsTrackedRows *tracked, int n, uint8_t *desc, const PsTrackedRows *out,
                        int32_t *srcIdx, int cap, int *nout, int *refill);
/* Diagnostic (no reference counterpart; profiles/scripts/track_close_times.py times the new launches alone with it):
 * ps_track_close_pairs with only the launches of the mask queued -- 1 the merge with the levels, 2 the placement, 4 the
 * descriptor rows, 8 the gather.  A launch reads what the launches before it left: call with 15 first. */
int ps_debug_track_close_passes(PsContext *ctx, PsTrackClose *tc, const PsOrbPyramids *pyr, const int32_t *slots, const PsTrackCloseParams *tp,
                                const PsTrackedRows *tracked, const PsTrackCandidates *cand, const int32_t *candFrame, int P, int capacity,
                                int outCapacity, const PsTrackCloseOut *out, int passes);

/* ---- Sub-pixel matching on patches: MatchingOnPatches (include/putslam/Matcher/MatchingOnPatches.h,
 * src/Matcher/MatchingOnPatches.cpp:14-246; configured by MatcherParameters::PatchesParams, matcher.h:295-304,362) -- the
 * Gauss-Newton alignment of a feature's patch from an old image in a new one.  Restated sequentially in tests/patches_ref.py;
 * every output is byte for byte the restatement's.  Eigen's Matrix3f::inverse(), its lazy 3 x 3 products
 * and cv::cvtColor are RESTATED, not compiled against the libraries: that reading is unpinned.
 * With h = (patchSize - 1) / 2, E = patchSize^2, element k running over rows i = int(y) - h .. int(y) + h and inside a row over
 * j = int(x) - h .. int(x) + h (int() truncates), I the grey image (one channel as it is, three by CV_RGB2GRAY: (c0 4899 +
 * c1 9617 + c2 1868 + 8192) >> 14), no multiply-add contracted:
 *   patch (:14-51), double: xs = x - int(x), ys = y - int(y); tl = (1-xs)(1-ys), tr = xs(1-ys), bl = (1-xs)ys, br = xs ys;
 *     patch[k] = ((tl I[i][j] + tr I[i][j+1]) + bl I[i+1][j]) + br I[i+1][j+1].
 *   gradient (:53-99), float: gx[k] = 0.5f (float)(I[i][j+1] - I[i][j-1]), gy[k] = 0.5f (float)(I[i+1][j] - I[i-1][j]), J = (gx, gy,
 *     1.f); H[a][b] += J[a] J[b] in k order from zero; invHessian = H^-1 by cof(i, j) = m(i1, j1) m(i2, j2) - m(i1, j2) m(i2, j1),
 *     det = (cof(0,0) m(0,0) + cof(1,0) m(1,0)) + cof(2,0) m(2,0), result(i, j) = cof(j, i) x (1.f / det); a zero determinant takes
 *     its IEEE course (NaN).  Row-major, 9 floats.
 *   alignment (:101-200): NaN invHessian[0] fails at once.  From (newX, newY), mean = 0.0, for up to maxIter steps: the gate
 *     isnan(newX) || isnan(newY) || newX < h || newX > cols - h || newY < h || newY > rows - h; the patch at (newX, newY); in k
 *     order diff = (float)((newPatch[k] - patch[k]) + mean), t0 -= diff gx[k], t1 -= diff gy[k], t2 -= diff (floats from 0.f);
 *     inc_r = (Inv[r][0] t0 + Inv[r][1] t1) + Inv[r][2] t2 for r = 0, 1; newX += (double)inc0, newY += (double)inc1; if
 *     (double)(inc0 inc0 + inc1 inc1) < minSqrtIncrement the point stops: moved too far if its squared distance from the start
 *     exceeds h h, else converged.
 * Two places where the reference reads outside its images are decided here: an OLD position must be finite with every tap inside
 * (int(x) - h - 1 >= 0, int(x) + h + 1 <= cols - 1, the same for y), else status 5; a NEW position that passes the gate while
 * int(newX) + h + 1 > cols - 1 or int(newY) + h + 1 > rows - 1 gets status 6.  `warping` (parsed, read nowhere) is not carried;
 * the narration to std::cout is not reproduced. */
enum {
    PS_PATCH_MAX_ITERATIONS = 0,    /* "Maximum iterations reached" (:193) */
    PS_PATCH_CONVERGED = 1,         /* the reference's true (:187) */
    PS_PATCH_NAN_HESSIAN = 2,       /* isnan(InvHessian(0,0)) (:108); position untouched */
    PS_PATCH_OUT_OF_IMAGE = 3,      /* the reference's gate (:139-154) */
    PS_PATCH_MOVED_TOO_FAR = 4,     /* (:176-180) */
    PS_PATCH_OLD_TAPS_OUTSIDE = 5,  /* this build: the old position's taps leave the old image, or a slot outside the set; position untouched */
    PS_PATCH_NEW_TAPS_OUTSIDE = 6   /* this build: the gate passed but the taps leave the new image */
};
enum { PS_PATCH_GIVEN_MODEL = 1 };  /* ps_patch_align reads the model arrays instead of building them from the old image */
typedef struct PsPatchParams {
    double minSqrtIncrement;     /* PatchesParams.minSqrtIncrement (the XML's minSqrtError) */
    int32_t patchSize;           /* odd, 3 .. 31 */
    int32_t maxIter;             /* 0 .. 1000 */
    int32_t flags;               /* PS_PATCH_GIVEN_MODEL */
    int32_t reserved;            /* 0 */
} PsPatchParams;
typedef struct PsPatchModel {    /* DEVICE pointers, P x capacity points each; NULL = not wanted */
    double *patch;               /* x E */
    float *gx, *gy;              /* x E */
    float *invHessian;           /* x 9, row-major */
} PsPatchModel;
size_t ps_abi_sizeof_patch_params(void);
size_t ps_abi_sizeof_patch_model(void);

/* computePatch + computeGradient (:14-99) for P sets of points, set p on frame slots[p] of `images`: pts P x capacity x 2 doubles
 * (x, y), counts P, status P x capacity bytes, all DEVICE.  status: 5 for a point whose taps leave the image (nothing of its
 * model is written), 2 for a NaN invHessian[0], else 1.  Nothing beyond a set's count is written; a count outside 0 .. capacity
 * leaves the set alone; a slot outside the set fails the set's points with status 5.  Bad params, NULL images / slots / pts /
 * counts / status (`model` itself may be NULL, as for ps_patch_align: the statuses alone), capacity < 1, P < 0, channels other than 1 or 3, an image above 8192 rows or columns: PS_ERR_BAD_ARG,
 * outputs untouched; P == 0 is PS_OK.  One wavefront per point.  Asynchronous on the context's stream; no scratch of the context. */
int ps_patch_models(PsContext *ctx, const PsImageSet *images, const int32_t *slots, const double *pts, const int32_t *counts, int P,
                    int capacity, const PsPatchParams *params, const PsPatchModel *model, uint8_t *status);
/* optimizeLocation (:101-200) for P pairs of frames: pairs P x 2 int32 (old slot, new slot; a pair may name one slot twice),
 * oldPts / newPts P x capacity x 2 doubles, counts P, status P x capacity bytes, iterations P x capacity int32 (the steps
 * applied), all DEVICE.  newPts is read as the starting guess and written as the reference leaves it: updated through the last
 * completed step, untouched for status 2 and 5.  Without PS_PATCH_GIVEN_MODEL the model is built from the old slot at oldPts and
 * written to the non-NULL arrays of `model` (which may itself be NULL); with it the four arrays are read, and neither the old
 * slot nor oldPts (may be NULL) is looked at.  Counts, slots (the ones read) and errors as for ps_patch_models.  Asynchronous. */
int ps_patch_align(PsContext *ctx, const PsImageSet *images, const int32_t *pairs, const double *oldPts, double *newPts,
                   const int32_t *counts, int P, int capacity, const PsPatchParams *params, const PsPatchModel *model, uint8_t *status,
                   int32_t *iterations);
/* The same for one image or one image pair and n points: HOST pointers, uploads and downloads included, synchronous.  Images
 * rows x cols x channels bytes, rowStride bytes apart (0 = dense); pts n x 2 doubles; patch n x E doubles; gx / gy n x E floats;
 * invHessian n x 9 floats; status n bytes; iterations n int32.  n == 0 is PS_OK.
 * ps_compute_patch: computePatch (:14-51); ps_compute_patch_gradient: computeGradient (:53-99), any of gx / gy / invHessian may
 * be NULL; ps_optimize_location: optimizeLocation (:101-200) on a given model (oldImg is not read, as in the reference, and may
 * be NULL); ps_optimize_locations: the three calls fused for n points. */
int ps_compute_patch(PsContext *ctx, const uint8_t *img, int rows, int cols, int channels, size_t rowStride, const double *pts, int n,
                     const PsPatchParams *params, double *patch, uint8_t *status);
int ps_compute_patch_gradient(PsContext *ctx, const uint8_t *img, int rows, int cols, int channels, size_t rowStride, const double *pts,
                              int n, const PsPatchParams *params, float *gx, float *gy, float *invHessian, uint8_t *status);
int ps_optimize_location(PsContext *ctx, const uint8_t *oldImg, const double *oldPatch, const uint8_t *newImg, int rows, int cols,
                         int channels, size_t rowStride, double *newPts, int n, const float *gx, const float *gy, const float *invHessian,
                         const PsPatchParams *params, uint8_t *status, int32_t *iterations);
int ps_optimize_locations(PsContext *ctx, const uint8_t *oldImg, const uint8_t *newImg, int rows, int cols, int channels,
                          size_t rowStride, const double *oldPts, double *newPts, int n, const PsPatchParams *params, uint8_t *status,
                          int32_t *iterations);

/* ---- Measurement uncertainty: the two per-feature steps of the frame loop before the data passes to the graph optimiser --
 * matcher->computeNormals / computeRGBGradients (src/PUTSLAM/PUTSLAM.cpp:826-837 for the measurements, :871-884 for the new
 * features) and the 3 x 3 information matrix FeaturesMap::addMeasurements (src/Map/featuresMap.cpp:251-285) and addFeatures
 * (:110-128) give every Edge3D.  The arithmetic is RGBD::computeNormal / computeRGBGradient (src/RGBD/RGBD.cpp:100-187, the
 * templates of RGBD.h:91-106), DepthSensorModel::computeCov (src/Grabber/depthSensorModel.cpp:27-36),
 * informationMatrixFromImageCoordinates (:55-59), uncertinatyFromNormal (:62-76), uncertinatyFromRGBGradient (:79-95) and
 * normalizeVector (:98-101), restated sequentially in tests/uncertainty_ref.py; every output is byte for byte the restatement's
 * (DESIGN.md section 8.16).  Eigen's fixed-size 3 x 3 inverse is RESTATED, not compiled against an Eigen: no Eigen was at hand,
 * so that reading is unpinned.
 * The rules, for a row with undistorted position (u, v) and point (X, Y, Z):
 *   pixel = ((int)u, (int)v), truncation (RGBD.h:93,104).  A NaN coordinate, or one whose truncation or its two neighbours do not
 *     fit an int, is undefined in the reference: here every double output of the row is NaN.  Every NaN written is the one pattern
 *     0x7FF8000000000000.
 *   point2Dto3D is ps_assemble_frames' arithmetic on a frame of the depth set as the dense image the reference holds.
 *   normal: the centre and its eight neighbours in the order of uidx / vidx; the neighbours with Z > 0 kept (the centre is not
 *     tested); differences in float, widened; cross products of cyclically adjacent kept vectors in double; their sum in list
 *     order divided by the count; norm = sqrt((x x + y y) + z z), three divisions.  Fewer than two kept neighbours: 0 / 0, NaN.
 *   gradient: 3-channel images only.  Outside the guard (u-1 > 0 && v-1 > 0 && u+1 < cols && v+1 < rows) the unnormalised
 *     (1, 1, 1).  The 3 x 3 patch is read as the reference reads it, at<uint16_t> on the 8-bit COLOUR image: the value at (r, c)
 *     is the little-endian 16-bit word at byte (v-1+r) x rowStride + (u-1) x 3 + 2 c of the frame.  gradx / grady are exact
 *     integers; the direction coord1 = (int(sqrt 2 sin a), int(sqrt 2 cos a)), a = atan2(grady, gradx) + pi / 2, and coord2 (a +
 *     pi) is taken by an integer rule off the diagonals -- coord1 = (sgn gradx if |gradx| > |grady| else 0, -sgn grady if |grady| >
 *     |gradx| else 0), coord2 = -coord1 -- and on the five ties ((0, 0) and |gradx| == |grady| in the four quadrants) from a table
 *     the HOST evaluates with its libm by the literal expression; then the selection ladder of :170-183 as written and the
 *     normalisation.
 *   info: model -1 the identity (useUncertainty off, or an uncertaintyModel the reference ignores); 0
 *     informationMatrixFromImageCoordinates(u, v, Z): computeCov((unsigned long)u, (unsigned long)v, Z).inverse(), a u or v that
 *     is negative, NaN or not below 2^64 giving a NaN matrix, z^2 = z z and z^3 = z z z (the correctly rounded powers of a float
 *     z; a libm's pow(z, 3.0) need not be); 1 uncertinatyFromNormal(normal).inverse(); 2
 *     uncertinatyFromRGBGradient(gradient).inverse().  Every 3 x 3 product is dense, (a0 b0 + a1 b1) + a2 b2, left to right;
 *     inverse(): cof(i, j) = m(i1, j1) m(i2, j2) - m(i1, j2) m(i2, j1), det = (cof(0,0) m(0,0) + cof(1,0) m(1,0)) + cof(2,0) m(2,0),
 *     result(i, j) = cof(j, i) x (1 / det).  Matrices are stored row-major, 9 doubles.
 * PsSensorModel: DepthSensorModel::Config (depthSensorModel.h:53-58).  The reference's file constructor never reads c1 and c0
 * (distVarCoefs[2], [3]): they are uninitialised there; the shipped Kinect file carries all four. */
typedef struct PsSensorModel {
    double fu, fv, cu, cv;       /* focalLength, focalAxis */
    double varU, varV;
    double c3, c2, c1, c0;       /* distVarCoefs[0 .. 3]: var(depth) = c3 z^3 + c2 z^2 + c1 z + c0 */
    double scaleUncertaintyNormal, scaleUncertaintyGradient;
} PsSensorModel;
typedef struct PsUncertaintyOut {  /* DEVICE pointers, F x capacity rows each; NULL = not wanted */
    double *normal;              /* x 3 */
    double *gradient;            /* x 3 */
    double *info;                /* x 9, row-major */
} PsUncertaintyOut;
typedef struct PsMeasurementEdgesOut {  /* DEVICE pointers, P x maxMatches rows each (count: P); NULL = not wanted */
    int32_t *count;              /* pair p's final inliers */
    int32_t *mapRow, *curRow;    /* queryIdx, trainIdx */
    float *uv;                   /* x 2: xyUndist of the frame's row (MapFeature::u, v) */
    double *position;            /* x 3: the frame's point widened -- the Edge3D measurement */
    double *normal, *gradient, *info;
} PsMeasurementEdgesOut;
size_t ps_abi_sizeof_sensor_model(void);
size_t ps_abi_sizeof_uncertainty_out(void);
size_t ps_abi_sizeof_measurement_edges_out(void);

/* DepthSensorModel::Config()'s defaults (depthSensorModel.h:53-58).  The two scale factors are 0: the reference's default
 * constructor leaves them unset.  Pure host; PS_ERR_BAD_ARG for NULL. */
int ps_sensor_model_default(PsSensorModel *out);

/* The addFeatures side (PUTSLAM.cpp:871-884, featuresMap.cpp:110-128) for F sets of rows, everything DEVICE resident: xy F x
 * capacity x 2 floats (the undistorted u, v: PsFrameRowsOut::xyUndist), pts F x capacity x 3 floats, counts F; imageFrame[f]
 * names the frame of `images` and of `depth` that row set f belongs to.  out->info with model 1 or 2 needs no normal / gradient
 * output; images may be NULL when neither the gradient nor model 2 is wanted.  A count outside 0 .. capacity: nothing written for
 * that set; imageFrame[f] outside either set: that set's rows are NaN; nothing is written beyond a count.  images->channels != 3
 * -> PS_ERR_UNSUPPORTED; NULL where an argument or array is needed, model outside -1 .. 2, strides that do not resolve, images of
 * another shape than the depth, capacity < 1, F outside 0 .. 65535 -> PS_ERR_BAD_ARG; capacity above PS_MAX_KPTS ->
 * PS_ERR_UNSUPPORTED; F == 0 is PS_OK.  One launch, asynchronous on the context's stream; uses no scratch of the context. */
int ps_feature_uncertainty(PsContext *ctx, const PsFrameGeometry *geometry, const PsSensorModel *sensor, int model,
                           const PsImageSet *images, const PsDepthSet *depth, const int32_t *imageFrame, const float *xy, const float *pts,
                           const int32_t *counts, int F, int capacity, const PsUncertaintyOut *out);

/* The addMeasurements side (matcher.cpp:769-794, then featuresMap.cpp:255-282) for the P pairs of a ps_map_pairs_device call: b
 * the PsMapBatch given to it, res its PsPairResults, xyUndist b->frames.numFrames x b->frames.maxKpts x 2 floats.  Pair p's final
 * inliers in match-list order (res->inlierMask's order is the order of inlierMatches) fill the first count[p] rows of every
 * wanted member of `out`; nothing is written beyond them.  The images' and the depth's frame is imageFrame[pairs[p][1]]
 * (imageFrame: b->frames.numFrames entries).  A pair with numMatches[p] <= 0 (no matches, or an overflow) or above b->maxMatches,
 * and a pair that names a frame outside its set, has count[p] = 0; a trainIdx outside 0 .. b->frames.maxKpts - 1 is not followed:
 * that row is NaN.  Errors as above (b's frame set by the rule of PsFrameSet, its points alone); P == 0 is PS_OK.  One launch, one
 * work-group per pair, no atomics -- the order is part of the result; asynchronous; no scratch. */
int ps_measurement_edges(PsContext *ctx, const PsFrameGeometry *geometry, const PsSensorModel *sensor, int model, const PsImageSet *images,
                         const PsDepthSet *depth, const int32_t *imageFrame, const PsMapBatch *b, const PsPairResults *res,
                         const float *xyUndist, const PsMeasurementEdgesOut *out);

/* The same for one frame: HOST pointers, uploads and downloads included, synchronous.  depth rows x cols uint16 with depthStep
 * bytes between rows, img rows x cols x 3 bytes with rowStride bytes between rows (0 = dense either); xy n x 2 floats, pts n x 3
 * floats; normal / gradient n x 3 doubles, info n x 9.  img may be NULL for models other than 2.  n above PS_MAX_KPTS ->
 * PS_ERR_UNSUPPORTED; n == 0 is PS_OK. */
int ps_compute_normals(PsContext *ctx, const PsFrameGeometry *geometry, const uint16_t *depth, int rows, int cols, size_t depthStep,
                       const float *xy, int n, double *normal);
int ps_compute_rgb_gradients(PsContext *ctx, const PsFrameGeometry *geometry, const uint8_t *img, int channels, size_t rowStride,
                             const uint16_t *depth, int rows, int cols, size_t depthStep, const float *xy, int n, double *gradient);
int ps_information_matrices(PsContext *ctx, const PsFrameGeometry *geometry, const PsSensorModel *sensor, int model, const uint8_t *img,
                            int channels, size_t rowStride, const uint16_t *depth, int rows, int cols, size_t depthStep, const float *xy,
                            const float *pts, int n, double *info);
/* Diagnostic (no reference counterpart; a CPU test holds the library's libm to the restatement's with it): the 5 x 4 table of the
 * gradient's ties -- rows (gradx, grady) = (0,0), (1,1), (-1,1), (-1,-1), (1,-1); columns coord1[0],
 * coord1[1], coord2[0], coord2[1] -- by the literal expression with this host's libm at magnitude k (the table the kernels get
 * is k = 1).  Pure host; k < 1 or NULL -> PS_ERR_BAD_ARG. */
int ps_debug_gradient_tie_table(int k, int32_t *table20);

#ifdef __cplusplus
}
#endif
#endif /* PUTSLAM_HIP_H_ */
