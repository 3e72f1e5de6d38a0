// capi_recorder.cpp -- a stand-in for the C ABI (include/putslam_hip.h) under the C++ drop-in, for tests/cpp/test_dropin_calls.cpp.
// Every ps_* function putslam_dropin.cpp references is defined here as a plain function: it writes one line with its name and every
// argument by value (structs field by field, input arrays as length:checksum, other pointers as null / ptr, never an address), fills
// its outputs from a fixed rule of the call's own sizes and returns PS_OK -- or, once, the status recorderFailNext() asked for.
// No GPU, no HIP call.  The three exclusion-rule builders, ps_predicted_level and ps_map_sphere_bound live in headers of the device
// unit in the library, so they are recorded like the rest.
#include <cstdio>
#include <cstring>
#include <iomanip>
#include <sstream>
#include <string>

#include "putslam_hip.h"

static std::string g_failName;
static int g_failCode = 0;

// the next call of `name` returns `code` (and fills nothing)
void recorderFailNext(const char *name, int code)
{
    g_failName = name;
    g_failCode = code;
}

namespace {

int failing(const char *name)
{
    if (g_failName != name) return 0;
    g_failName.clear();
    return g_failCode;
}

struct Line {
    std::ostringstream o;
    explicit Line(const char *fn)
    {
        o << std::setprecision(17) << "  [capi] " << fn;
    }
    template <class T> Line &a(const char *k, const T &v)
    {
        o << ' ' << k << '=' << v;
        return *this;
    }
    ~Line()
    {
        o << '\n';
        std::fputs(o.str().c_str(), stdout);
    }
};

const char *ptr(const void *p) { return p ? "ptr" : "null"; }

// length:checksum (FNV-1a) of `rows` runs of `bytes` bytes, `stride` apart
std::string arr(const void *p, size_t rows, size_t bytes, size_t stride)
{
    std::ostringstream o;
    o << rows << 'x' << bytes << ':';
    if (rows == 0 || bytes == 0) return o.str();
    if (!p) return o.str() + "null";
    uint64_t h = 1469598103934665603ull;
    for (size_t r = 0; r < rows; ++r) {
        const unsigned char *b = static_cast<const unsigned char *>(p) + r * stride;
        for (size_t i = 0; i < bytes; ++i) h = (h ^ b[i]) * 1099511628211ull;
    }
    o << std::hex << h;
    return o.str();
}
std::string arr(const void *p, size_t n, size_t elem) { return arr(p, n, elem, elem); }

template <class T> std::string vec(const T *v, int n)
{
    if (!v) return "null";
    std::ostringstream o;
    o << std::setprecision(17) << '(';
    for (int i = 0; i < n; ++i) o << (i ? "," : "") << v[i];
    o << ')';
    return o.str();
}

std::string str(const PsRansacParams *p)
{
    if (!p) return "null";
    std::ostringstream o;
    o << std::setprecision(17) << "{verbose=" << p->verbose << " errorVersion=" << p->errorVersion << " errorVersionVO=" << p->errorVersionVO
      << " errorVersionMap=" << p->errorVersionMap << " inlierThresholdEuclidean=" << p->inlierThresholdEuclidean
      << " inlierThresholdReprojection=" << p->inlierThresholdReprojection << " inlierThresholdMahalanobis=" << p->inlierThresholdMahalanobis
      << " minimalInlierRatioThreshold=" << p->minimalInlierRatioThreshold << " minimalNumberOfMatches=" << p->minimalNumberOfMatches
      << " usedPairs=" << p->usedPairs << " iterationCount=" << p->iterationCount << '}';
    return o.str();
}
std::string str(const PsRansacConfig *c)
{
    if (!c) return "null";
    std::ostringstream o;
    o << "{estimator=" << c->estimator << " numHypotheses=" << c->numHypotheses << " seed=" << c->seed << " sampleIdx=" << ptr(c->sampleIdx) << '}';
    return o.str();
}
std::string str(const PsKltParams *p)
{
    if (!p) return "null";
    std::ostringstream o;
    o << std::setprecision(17) << "{eps=" << p->eps << " minEigThreshold=" << p->minEigThreshold << " winSize=" << p->winSize
      << " maxLevels=" << p->maxLevels << " maxCount=" << p->maxCount << " flags=" << p->flags << '}';
    return o.str();
}
std::string str(const PsOrbDetectParams *p)
{
    if (!p) return "null";
    std::ostringstream o;
    o << std::setprecision(17) << "{nFeatures=" << p->nFeatures << " scaleFactor=" << p->scaleFactor << " nLevels=" << p->nLevels
      << " fastThreshold=" << p->fastThreshold << " gridRows=" << p->gridRows << " gridCols=" << p->gridCols
      << " maximalTrackedFeatures=" << p->maximalTrackedFeatures << " reserved=" << p->reserved << '}';
    return o.str();
}
std::string str(const PsDetectParams *p)
{
    if (!p) return "null";
    std::ostringstream o;
    o << "{threshold=" << p->threshold << " nonmaxSuppression=" << p->nonmaxSuppression << " gridRows=" << p->gridRows << " gridCols=" << p->gridCols
      << " maximalTrackedFeatures=" << p->maximalTrackedFeatures << " reserved=" << p->reserved << '}';
    return o.str();
}
std::string str(const PsOrbParams *p)
{
    if (!p) return "null";
    std::ostringstream o;
    o << std::setprecision(17) << "{scaleFactor=" << p->scaleFactor << " nLevels=" << p->nLevels << " reserved=" << vec(p->reserved, 2) << '}';
    return o.str();
}
std::string str(const PsFrontEndParams *p)
{
    if (!p) return "null";
    std::ostringstream o;
    o << std::setprecision(17) << "{detect=" << str(&p->detect) << " describe=" << str(&p->describe) << " DBScanEps=" << p->DBScanEps << '}';
    return o.str();
}
std::string str(const PsFrameGeometry *g)
{
    if (!g) return "null";
    std::ostringstream o;
    o << std::setprecision(17) << "{K=" << vec(g->K, 9) << " dist5=" << vec(g->dist5, 5) << " depthImageScale=" << g->depthImageScale << '}';
    return o.str();
}
std::string str(const PsTrackVoParams *p)
{
    if (!p) return "null";
    std::ostringstream o;
    o << std::setprecision(17) << "{trackingErrorThreshold=" << p->trackingErrorThreshold
      << " minimalReprojDistanceNewTrackingFeatures=" << p->minimalReprojDistanceNewTrackingFeatures
      << " removeTooCloseFeatures=" << p->removeTooCloseFeatures << " reserved=" << p->reserved << '}';
    return o.str();
}
std::string str(const PsTrackCloseParams *p)
{
    if (!p) return "null";
    std::ostringstream o;
    o << std::setprecision(17) << "{minimalReprojDistanceNewTrackingFeatures=" << p->minimalReprojDistanceNewTrackingFeatures
      << " minimalTrackedFeatures=" << p->minimalTrackedFeatures << " removeTooCloseFeatures=" << p->removeTooCloseFeatures << '}';
    return o.str();
}
std::string str(const PsExclusionRule *r)
{
    if (!r) return "null";
    std::ostringstream o;
    o << std::setprecision(17) << "{bound3=" << r->bound3 << " bound2=" << r->bound2 << " depthMin=" << r->depthMin << " depthMax=" << r->depthMax
      << " form3=" << r->form3 << " form2=" << r->form2 << " mode=" << r->mode << " maxKeep=" << r->maxKeep << " depthGate=" << r->depthGate
      << " reserved=" << r->reserved << '}';
    return o.str();
}
// the image's pixel bytes, row by row (the padding of a stepped image is not read)
std::string image(const void *p, int rows, int cols, int channels, size_t step, size_t elem)
{
    if (rows <= 0 || cols <= 0 || channels <= 0) return "none";
    return arr(p, (size_t)rows, (size_t)cols * (size_t)channels * elem, step);
}

// ---- the fixed rules the outputs follow ----
int min3(int a) { return a < 3 ? (a < 0 ? 0 : a) : 3; }
int evens(int n) { return min3((n + 1) / 2); } // how many of 0, 2, 4 stay below n
void fillPose(float *pose, float t)
{
    if (!pose) return;
    for (int i = 0; i < 16; ++i) pose[i] = i % 5 == 0 ? 1.0f : 0.0f;
    pose[12] = 0.01f * t;
    pose[13] = 0.02f;
    pose[14] = -0.03f;
}
void fillStats(PsRansacStats *st, int m, int inl)
{
    if (!st) return;
    std::memset(st, 0, sizeof *st);
    st->numMatchesIn = st->numMatchesValid = m;
    st->bestHypothesis = 1;
    st->bestInlierCount = st->numInliers = inl;
    st->iterationsRun = 7;
    st->accepted = 1;
    st->bestInlierRatio = 0.5f;
    st->pointInlierRatio = 0.75;
}
void fillXY(float *xy, int j)
{
    if (!xy) return;
    xy[2 * j] = (float)j + 0.5f;
    xy[2 * j + 1] = 2.0f * (float)j;
}
void fillPts(float *p, int j)
{
    if (!p) return;
    p[3 * j] = 0.1f * (float)j;
    p[3 * j + 1] = 0.1f * (float)(j + 1);
    p[3 * j + 2] = 1.0f + (float)j;
}
void fillRows(uint8_t *desc, int n)
{
    for (int i = 0; desc && i < n * 32; ++i) desc[i] = (uint8_t)(i * 7 + 1);
}
PsDMatch dm(int q, int t, float d)
{
    PsDMatch m;
    m.queryIdx = q;
    m.trainIdx = t;
    m.imgIdx = 0;
    m.distance = d;
    return m;
}

char g_ctx; // what a PsContext * points at
int g_streams = 0;

} // namespace

struct PsVoStream {
    int id, frames, popped, lastN;
};

extern "C" {

int ps_context_create(int device, PsContext **out)
{
    Line("ps_context_create").a("device", device).a("out", ptr(out));
    if (int rc = failing("ps_context_create")) return rc;
    *out = reinterpret_cast<PsContext *>(&g_ctx);
    return PS_OK;
}
void ps_context_destroy(PsContext *ctx) { Line("ps_context_destroy").a("ctx", ptr(ctx)); }
int ps_context_device(const PsContext *ctx)
{
    Line("ps_context_device").a("ctx", ptr(ctx));
    return 0;
}
void *ps_context_stream(PsContext *ctx)
{
    Line("ps_context_stream").a("ctx", ptr(ctx));
    return nullptr;
}
int ps_context_synchronize(PsContext *ctx)
{
    Line("ps_context_synchronize").a("ctx", ptr(ctx));
    return failing("ps_context_synchronize");
}
const char *ps_last_error(const PsContext *ctx)
{
    Line("ps_last_error").a("ctx", ptr(ctx));
    return "the recorder's error text";
}

int ps_ransac_rigid3d(PsContext *ctx, const PsRansacParams *params, const PsRansacConfig *cfg, const float *K, const float *prev, int nprev,
                      const float *cur, int ncur, const PsDMatch *matches, int m, float *pose, PsDMatch *inliers, int *ninl, uint8_t *mask,
                      PsRansacStats *stats)
{
    Line("ps_ransac_rigid3d").a("ctx", ptr(ctx)).a("params", str(params)).a("cfg", str(cfg)).a("K", vec(K, 9)).a("prev", arr(prev, nprev, 12))
        .a("cur", arr(cur, ncur, 12)).a("matches", arr(matches, m, 16)).a("pose", ptr(pose)).a("inliers", ptr(inliers)).a("ninl", ptr(ninl))
        .a("mask", ptr(mask)).a("stats", ptr(stats));
    if (int rc = failing("ps_ransac_rigid3d")) return rc;
    const int k = evens(m);
    for (int j = 0; j < k; ++j) inliers[j] = matches[2 * j];
    *ninl = k;
    fillPose(pose, (float)m);
    fillStats(stats, m, k);
    return PS_OK;
}

int ps_keypoints2Dto3D(PsContext *ctx, const float *xy, int n, const uint16_t *depth, int rows, int cols, size_t depthStep, const float *K,
                       double depthImageScale, float *out)
{
    Line("ps_keypoints2Dto3D").a("ctx", ptr(ctx)).a("xy", arr(xy, n, 8)).a("depth", image(depth, rows, cols, 1, depthStep, 2)).a("rows", rows)
        .a("cols", cols).a("depthStep", depthStep).a("K", vec(K, 9)).a("depthImageScale", depthImageScale).a("out", ptr(out));
    if (int rc = failing("ps_keypoints2Dto3D")) return rc;
    for (int j = 0; j < n; ++j) {
        out[3 * j] = xy[2 * j];
        out[3 * j + 1] = xy[2 * j + 1];
        out[3 * j + 2] = (float)(j + 1);
    }
    return PS_OK;
}

int ps_dbscan_thin(PsContext *ctx, const float *xy, size_t xyStride, const int32_t *octave, size_t octaveStride, int n, double eps, int minPts,
                   int featuresFromCluster, int32_t *keptIdx, int *nkept)
{
    Line("ps_dbscan_thin").a("ctx", ptr(ctx)).a("xy", arr(xy, n, 8, xyStride)).a("xyStride", xyStride).a("octave", arr(octave, n, 4, octaveStride))
        .a("octaveStride", octaveStride).a("eps", eps).a("minPts", minPts).a("featuresFromCluster", featuresFromCluster)
        .a("keptIdx", ptr(keptIdx)).a("nkept", ptr(nkept));
    if (int rc = failing("ps_dbscan_thin")) return rc;
    *nkept = (n + 1) / 2;
    for (int j = 0; j < *nkept; ++j) keptIdx[j] = 2 * j;
    return PS_OK;
}

int ps_exclusion_rule_new_map_features(double minEuclideanDistanceOfFeatures, double minImageDistanceOfFeatures, int maxOnceFeatureAdd,
                                       PsExclusionRule *rule)
{
    Line("ps_exclusion_rule_new_map_features").a("minEuclideanDistanceOfFeatures", minEuclideanDistanceOfFeatures)
        .a("minImageDistanceOfFeatures", minImageDistanceOfFeatures).a("maxOnceFeatureAdd", maxOnceFeatureAdd).a("rule", ptr(rule));
    std::memset(rule, 0, sizeof *rule);
    rule->bound3 = minEuclideanDistanceOfFeatures;
    rule->bound2 = minImageDistanceOfFeatures;
    rule->form3 = PS_EXCL_F32;
    rule->form2 = PS_EXCL_F32;
    rule->mode = PS_EXCL_GREEDY;
    rule->maxKeep = maxOnceFeatureAdd;
    return PS_OK;
}
int ps_exclusion_rule_merge_tracked(double minimalReprojDistanceNewTrackingFeatures, PsExclusionRule *rule)
{
    Line("ps_exclusion_rule_merge_tracked").a("minimalReprojDistanceNewTrackingFeatures", minimalReprojDistanceNewTrackingFeatures)
        .a("rule", ptr(rule));
    std::memset(rule, 0, sizeof *rule);
    rule->bound2 = minimalReprojDistanceNewTrackingFeatures;
    rule->form2 = PS_EXCL_F64;
    rule->mode = PS_EXCL_GREEDY;
    rule->maxKeep = -1;
    return PS_OK;
}
int ps_exclusion_rule_too_close(double minimalEuclidDistanceNewTrackingFeatures, double minimalReprojDistanceNewTrackingFeatures,
                                PsExclusionRule *rule)
{
    Line("ps_exclusion_rule_too_close").a("minimalEuclidDistanceNewTrackingFeatures", minimalEuclidDistanceNewTrackingFeatures)
        .a("minimalReprojDistanceNewTrackingFeatures", minimalReprojDistanceNewTrackingFeatures).a("rule", ptr(rule));
    std::memset(rule, 0, sizeof *rule);
    rule->bound3 = minimalEuclidDistanceNewTrackingFeatures;
    rule->bound2 = minimalReprojDistanceNewTrackingFeatures;
    rule->form3 = PS_EXCL_F64;
    rule->form2 = PS_EXCL_F64;
    rule->mode = PS_EXCL_ALL_EARLIER;
    rule->maxKeep = -1;
    return PS_OK;
}
int ps_exclude(PsContext *ctx, const PsExclusionRule *rule, const float *cand3, const float *cand2, int n, const float *exist3, const float *exist2,
               int m, int32_t *keptIdx, int *nkept)
{
    Line("ps_exclude").a("ctx", ptr(ctx)).a("rule", str(rule)).a("cand3", cand3 ? arr(cand3, n, 12) : "null").a("cand2", arr(cand2, n, 8))
        .a("exist3", exist3 ? arr(exist3, m, 12) : "null").a("exist2", exist2 ? arr(exist2, m, 8) : "null").a("m", m).a("keptIdx", ptr(keptIdx))
        .a("nkept", ptr(nkept));
    if (int rc = failing("ps_exclude")) return rc;
    *nkept = (n + 1) / 2;
    for (int j = 0; j < *nkept; ++j) keptIdx[j] = 2 * j;
    return PS_OK;
}

int ps_remove_image_distortion(PsContext *ctx, const float *xy, int n, const float *K, const double *dist5, float *out)
{
    Line("ps_remove_image_distortion").a("ctx", ptr(ctx)).a("xy", arr(xy, n, 8)).a("K", vec(K, 9)).a("dist5", vec(dist5, 5)).a("out", ptr(out));
    if (int rc = failing("ps_remove_image_distortion")) return rc;
    for (int j = 0; j < n; ++j) {
        out[2 * j] = xy[2 * j] + 0.25f;
        out[2 * j + 1] = xy[2 * j + 1] - 0.25f;
    }
    return PS_OK;
}
int ps_points3Dto2D(PsContext *ctx, const float *xyz, int n, const float *K, float *uv)
{
    Line("ps_points3Dto2D").a("ctx", ptr(ctx)).a("xyz", arr(xyz, n, 12)).a("K", vec(K, 9)).a("uv", ptr(uv));
    if (int rc = failing("ps_points3Dto2D")) return rc;
    for (int j = 0; j < n; ++j) {
        uv[2 * j] = xyz[3 * j] + xyz[3 * j + 2];
        uv[2 * j + 1] = xyz[3 * j + 1] + xyz[3 * j + 2];
    }
    return PS_OK;
}
int ps_kabsch_f64(PsContext *ctx, const double *A, const double *B, int n, int ld, double *T)
{
    Line("ps_kabsch_f64").a("ctx", ptr(ctx)).a("A", arr(A, (size_t)3 * n, 8)).a("B", arr(B, (size_t)3 * n, 8)).a("n", n).a("ld", ld).a("T", ptr(T));
    if (int rc = failing("ps_kabsch_f64")) return rc;
    for (int i = 0; i < 16; ++i) T[i] = i % 5 == 0 ? 1.0 : 0.0;
    T[12] = (double)n;
    return PS_OK;
}

// ---- resident frames and the pipelined stream: one counter per stream stands for the frames it holds ----
int ps_vo_stream_create(PsContext *ctx, int maxKpts, PsVoStream **out)
{
    Line("ps_vo_stream_create").a("ctx", ptr(ctx)).a("maxKpts", maxKpts).a("out", ptr(out)).a("id", g_streams + 1);
    if (int rc = failing("ps_vo_stream_create")) return rc;
    *out = new PsVoStream{++g_streams, 0, 0, 0};
    return PS_OK;
}
void ps_vo_stream_destroy(PsVoStream *s)
{
    Line("ps_vo_stream_destroy").a("s", s ? s->id : 0);
    delete s;
}
int ps_vo_stream_reset(PsVoStream *s)
{
    Line("ps_vo_stream_reset").a("s", s->id);
    s->frames = s->popped = 0;
    return PS_OK;
}
int ps_vo_stream_push(PsVoStream *s, const PsRansacParams *params, const PsRansacConfig *cfg, const float *K, const uint8_t *desc, size_t descStep,
                      const float *pts, int n, PsDMatch *matches, int *nmatches, uint8_t *inlierMask, float *pose, PsRansacStats *stats)
{
    Line("ps_vo_stream_push").a("s", s->id).a("params", str(params)).a("cfg", str(cfg)).a("K", vec(K, 9)).a("desc", arr(desc, n, 32, descStep))
        .a("descStep", descStep).a("pts", arr(pts, n, 12)).a("matches", ptr(matches)).a("nmatches", ptr(nmatches))
        .a("inlierMask", ptr(inlierMask)).a("pose", ptr(pose)).a("stats", ptr(stats));
    if (int rc = failing("ps_vo_stream_push")) return rc;
    const int k = s->frames > 0 ? min3(n) : 0;
    int inl = 0;
    for (int j = 0; j < k; ++j) {
        matches[j] = dm(j, (2 * j) % n, (float)j + 0.5f);
        inlierMask[j] = (uint8_t)(j % 2 == 0);
        inl += inlierMask[j];
    }
    *nmatches = k;
    fillPose(pose, (float)n);
    fillStats(stats, k, inl);
    ++s->frames;
    return PS_OK;
}
int ps_vo_stream_set_result_mode(PsVoStream *s, int mode)
{
    Line("ps_vo_stream_set_result_mode").a("s", s->id).a("mode", mode);
    return PS_OK;
}
int ps_vo_stream_configure_async(PsVoStream *s, const PsRansacParams *params, const PsRansacConfig *cfg, const float *K, int chunkFrames, int lanes)
{
    Line("ps_vo_stream_configure_async").a("s", s->id).a("params", str(params)).a("cfg", str(cfg)).a("K", vec(K, 9)).a("chunkFrames", chunkFrames)
        .a("lanes", lanes);
    return failing("ps_vo_stream_configure_async");
}
int ps_vo_stream_push_async(PsVoStream *s, const uint8_t *desc, size_t descStep, const float *pts, int n)
{
    Line("ps_vo_stream_push_async").a("s", s->id).a("desc", arr(desc, n, 32, descStep)).a("descStep", descStep).a("pts", arr(pts, n, 12));
    if (int rc = failing("ps_vo_stream_push_async")) return rc;
    ++s->frames;
    s->lastN = n;
    return PS_OK;
}
int ps_vo_stream_pending(const PsVoStream *s)
{
    const int pending = s->frames > 0 ? s->frames - 1 - s->popped : 0;
    Line("ps_vo_stream_pending").a("s", s->id).a("returns", pending);
    return pending;
}
int ps_vo_stream_flush(PsVoStream *s)
{
    Line("ps_vo_stream_flush").a("s", s->id);
    return failing("ps_vo_stream_flush");
}
int ps_vo_stream_pop(PsVoStream *s, int wait, PsDMatch *matches, int *nmatches, uint8_t *inlierMask, float *pose, PsRansacStats *stats)
{
    Line("ps_vo_stream_pop").a("s", s->id).a("wait", wait).a("matches", ptr(matches)).a("nmatches", ptr(nmatches)).a("inlierMask", ptr(inlierMask))
        .a("pose", ptr(pose)).a("stats", ptr(stats));
    if (int rc = failing("ps_vo_stream_pop")) return rc;
    if (s->frames - 1 - s->popped <= 0) {
        *nmatches = -1;
        return PS_OK;
    }
    const int k = min3(s->lastN);
    for (int j = 0; j < k; ++j) {
        matches[j] = dm(j, j, (float)(s->popped + j));
        inlierMask[j] = 1;
    }
    *nmatches = k;
    fillPose(pose, (float)s->popped);
    fillStats(stats, k, k);
    ++s->popped;
    return PS_OK;
}

// ---- matching ----
int ps_match_hamming256(PsContext *ctx, const uint8_t *query, int nq, size_t qstep, const uint8_t *train, int nt, size_t tstep, PsDMatch *out,
                        int *nout)
{
    Line("ps_match_hamming256").a("ctx", ptr(ctx)).a("query", arr(query, nq, 32, qstep)).a("qstep", qstep).a("train", arr(train, nt, 32, tstep))
        .a("tstep", tstep).a("out", ptr(out)).a("nout", ptr(nout));
    if (int rc = failing("ps_match_hamming256")) return rc;
    const int k = min3(nq < nt ? nq : nt);
    for (int j = 0; j < k; ++j) out[j] = dm(j, (2 * j) % nt, (float)(10 + j));
    *nout = k;
    return PS_OK;
}
int ps_match_l2_f32(PsContext *ctx, const float *query, int nq, size_t qstepBytes, const float *train, int nt, size_t tstepBytes, int dim, PsDMatch *out,
                    int *nout)
{
    Line("ps_match_l2_f32").a("ctx", ptr(ctx)).a("query", arr(query, nq, (size_t)dim * 4, qstepBytes)).a("qstepBytes", qstepBytes)
        .a("train", arr(train, nt, (size_t)dim * 4, tstepBytes)).a("tstepBytes", tstepBytes).a("dim", dim).a("out", ptr(out)).a("nout", ptr(nout));
    if (int rc = failing("ps_match_l2_f32")) return rc;
    const int k = min3(nq < nt ? nq : nt);
    for (int j = 0; j < k; ++j) out[j] = dm(j, (2 * j) % nt, 0.25f * (float)j);
    *nout = k;
    return PS_OK;
}
int ps_predicted_level(int octave, double detDist, double curDist)
{
    const int level = octave + (curDist > detDist ? 1 : 0);
    Line("ps_predicted_level").a("octave", octave).a("detDist", detDist).a("curDist", curDist).a("returns", level);
    return level;
}
float ps_map_sphere_bound(double sphereRadius)
{
    Line("ps_map_sphere_bound").a("sphereRadius", sphereRadius);
    return (float)(sphereRadius * sphereRadius);
}
// (PS_ERR_ALLOC asked for: the call reports four rows more than it was given room for, as an overflowing call does)
static int mapMatches(const char *name, int nmap, int ncur, PsDMatch *out, int cap, int *nout)
{
    if (int rc = failing(name)) {
        if (rc == PS_ERR_ALLOC) *nout = cap + 4;
        return rc;
    }
    const int k = min3(cap < nmap ? cap : nmap);
    for (int j = 0; j < k; ++j) out[j] = dm(j, j % ncur, (float)j);
    *nout = k;
    return PS_OK;
}
int ps_match_xyz(PsContext *ctx, const float *mapPos, const uint8_t *mapDesc, size_t mapDescStep, const int32_t *mapLevel, int nmap, const float *curPos,
                 const uint8_t *curDesc, size_t curDescStep, const int32_t *curLevel, int ncur, double sphereRadius, double acceptRatio, PsDMatch *out,
                 int cap, int *nout)
{
    Line("ps_match_xyz").a("ctx", ptr(ctx)).a("mapPos", arr(mapPos, nmap, 12)).a("mapDesc", arr(mapDesc, nmap, 32, mapDescStep))
        .a("mapDescStep", mapDescStep).a("mapLevel", arr(mapLevel, nmap, 4)).a("curPos", arr(curPos, ncur, 12))
        .a("curDesc", arr(curDesc, ncur, 32, curDescStep)).a("curDescStep", curDescStep).a("curLevel", arr(curLevel, ncur, 4))
        .a("sphereRadius", sphereRadius).a("acceptRatio", acceptRatio).a("out", ptr(out)).a("cap", cap).a("nout", ptr(nout));
    return mapMatches("ps_match_xyz", nmap, ncur, out, cap, nout);
}
int ps_match_xyz_l2_f32(PsContext *ctx, const float *mapPos, const float *mapDesc, size_t mapDescStepBytes, const int32_t *mapLevel, int nmap,
                        const float *curPos, const float *curDesc, size_t curDescStepBytes, const int32_t *curLevel, int ncur, int dim,
                        double sphereRadius, double acceptRatio, PsDMatch *out, int cap, int *nout)
{
    Line("ps_match_xyz_l2_f32").a("ctx", ptr(ctx)).a("mapPos", arr(mapPos, nmap, 12)).a("mapDesc", arr(mapDesc, nmap, (size_t)dim * 4, mapDescStepBytes))
        .a("mapDescStepBytes", mapDescStepBytes).a("mapLevel", arr(mapLevel, nmap, 4)).a("curPos", arr(curPos, ncur, 12))
        .a("curDesc", arr(curDesc, ncur, (size_t)dim * 4, curDescStepBytes)).a("curDescStepBytes", curDescStepBytes)
        .a("curLevel", arr(curLevel, ncur, 4)).a("dim", dim).a("sphereRadius", sphereRadius).a("acceptRatio", acceptRatio).a("out", ptr(out))
        .a("cap", cap).a("nout", ptr(nout));
    return mapMatches("ps_match_xyz_l2_f32", nmap, ncur, out, cap, nout);
}
// matchXYZLadder's calls: the driver leaves the ladder out (its block lives in device memory), these only have to link
int ps_map_pairs_device(PsContext *ctx, const PsRansacParams *params, const PsRansacConfig *cfg, const float *K, const PsMapBatch *b,
                        const PsPairResults *out)
{
    Line("ps_map_pairs_device").a("ctx", ptr(ctx)).a("params", str(params)).a("cfg", str(cfg)).a("K", vec(K, 9)).a("b", ptr(b)).a("out", ptr(out));
    return PS_ERR_UNSUPPORTED;
}
int ps_map_pairs_l2_device(PsContext *ctx, const PsRansacParams *params, const PsRansacConfig *cfg, const float *K, const PsMapBatchF32 *b,
                           const PsPairResults *out)
{
    Line("ps_map_pairs_l2_device").a("ctx", ptr(ctx)).a("params", str(params)).a("cfg", str(cfg)).a("K", vec(K, 9)).a("b", ptr(b)).a("out", ptr(out));
    return PS_ERR_UNSUPPORTED;
}

// ---- the image front end ----
int ps_perform_tracking(PsContext *ctx, const uint8_t *prevImg, const uint8_t *nextImg, int rows, int cols, int channels, size_t rowStride,
                        const float *prevPts, float *nextPts, int n, const PsKltParams *params, double trackingErrorThreshold,
                        double minimalReprojDistance, uint8_t *status, float *err, PsDMatch *matches, int *numMatches, float *keptPts, int32_t *keptIdx)
{
    Line("ps_perform_tracking").a("ctx", ptr(ctx)).a("prevImg", image(prevImg, rows, cols, channels, rowStride, 1))
        .a("nextImg", image(nextImg, rows, cols, channels, rowStride, 1)).a("rows", rows).a("cols", cols).a("channels", channels)
        .a("rowStride", rowStride).a("prevPts", arr(prevPts, n, 8)).a("nextPts", arr(nextPts, n, 8)).a("params", str(params))
        .a("trackingErrorThreshold", trackingErrorThreshold).a("minimalReprojDistance", minimalReprojDistance).a("status", ptr(status))
        .a("err", ptr(err)).a("matches", ptr(matches)).a("numMatches", ptr(numMatches)).a("keptPts", ptr(keptPts)).a("keptIdx", ptr(keptIdx));
    if (int rc = failing("ps_perform_tracking")) return rc;
    const int k = evens(n);
    for (int j = 0; j < k; ++j) {
        keptIdx[j] = 2 * j;
        fillXY(keptPts, j);
        matches[j] = dm(2 * j, j, 0.0f);
    }
    *numMatches = k;
    return PS_OK;
}
int ps_detect_features(PsContext *ctx, const uint8_t *img, int rows, int cols, int channels, size_t rowStride, const PsDetectParams *params, float *xy,
                       float *response, int cap, int *nout)
{
    Line("ps_detect_features").a("ctx", ptr(ctx)).a("img", image(img, rows, cols, channels, rowStride, 1)).a("rows", rows).a("cols", cols)
        .a("channels", channels).a("rowStride", rowStride).a("params", str(params)).a("xy", ptr(xy)).a("response", ptr(response)).a("cap", cap)
        .a("nout", ptr(nout));
    if (int rc = failing("ps_detect_features")) return rc;
    const int k = min3(cap);
    for (int j = 0; j < k; ++j) {
        fillXY(xy, j);
        response[j] = 10.0f - (float)j;
    }
    *nout = k;
    return PS_OK;
}
int ps_detect_features_orb(PsContext *ctx, const uint8_t *img, int rows, int cols, int channels, size_t rowStride, const PsOrbDetectParams *params,
                           float *xy, float *response, float *angle, int32_t *octave, int cap, int *nout)
{
    Line("ps_detect_features_orb").a("ctx", ptr(ctx)).a("img", image(img, rows, cols, channels, rowStride, 1)).a("rows", rows).a("cols", cols)
        .a("channels", channels).a("rowStride", rowStride).a("params", str(params)).a("xy", ptr(xy)).a("response", ptr(response))
        .a("angle", ptr(angle)).a("octave", ptr(octave)).a("cap", cap).a("nout", ptr(nout));
    if (int rc = failing("ps_detect_features_orb")) return rc;
    const int k = min3(cap);
    for (int j = 0; j < k; ++j) {
        fillXY(xy, j);
        response[j] = 10.0f - (float)j;
        angle[j] = 30.0f * (float)j;
        octave[j] = j % 3;
    }
    *nout = k;
    return PS_OK;
}
int ps_describe_features(PsContext *ctx, const uint8_t *img, int rows, int cols, int channels, size_t rowStride, const PsOrbParams *params,
                         const int8_t *pattern1024, const float *xy, const float *angle, const int32_t *octave, int n, uint8_t *desc, int32_t *keptIdx,
                         int *nout)
{
    Line("ps_describe_features").a("ctx", ptr(ctx)).a("img", image(img, rows, cols, channels, rowStride, 1)).a("rows", rows).a("cols", cols)
        .a("channels", channels).a("rowStride", rowStride).a("params", str(params)).a("pattern1024", ptr(pattern1024)).a("xy", arr(xy, n, 8))
        .a("angle", arr(angle, n, 4)).a("octave", arr(octave, n, 4)).a("desc", ptr(desc)).a("keptIdx", ptr(keptIdx)).a("nout", ptr(nout));
    if (int rc = failing("ps_describe_features")) return rc;
    const int k = evens(n);
    for (int j = 0; j < k; ++j) keptIdx[j] = 2 * j;
    fillRows(desc, k);
    *nout = k;
    return PS_OK;
}
int ps_front_end_frame(PsContext *ctx, const uint8_t *img, const uint16_t *depth, int rows, int cols, int channels, size_t rowStride, size_t depthStep,
                       const PsFrontEndParams *params, const int8_t *pattern1024, const PsFrameGeometry *geometry, uint8_t *desc,
                       const PsFrameRowsOut *out, int cap, int *nout)
{
    Line("ps_front_end_frame").a("ctx", ptr(ctx)).a("img", image(img, rows, cols, channels, rowStride, 1))
        .a("depth", image(depth, rows, cols, 1, depthStep, 2)).a("rows", rows).a("cols", cols).a("channels", channels).a("rowStride", rowStride)
        .a("depthStep", depthStep).a("params", str(params)).a("pattern1024", ptr(pattern1024)).a("geometry", str(geometry)).a("desc", ptr(desc))
        .a("out.pts", ptr(out->pts)).a("out.nkpts", ptr(out->nkpts)).a("out.xy", ptr(out->xy)).a("out.xyUndist", ptr(out->xyUndist))
        .a("out.angle", ptr(out->angle)).a("out.response", ptr(out->response)).a("out.octave", ptr(out->octave)).a("out.srcIdx", ptr(out->srcIdx))
        .a("out.detDist", ptr(out->detDist)).a("out.angleIn", ptr(out->angleIn)).a("out.responseIn", ptr(out->responseIn))
        .a("out.octaveIn", ptr(out->octaveIn)).a("cap", cap).a("nout", ptr(nout));
    if (int rc = failing("ps_front_end_frame")) return rc;
    const int k = min3(cap);
    for (int j = 0; j < k; ++j) {
        fillPts(out->pts, j);
        fillXY(out->xy, j);
        fillXY(out->xyUndist, j);
        if (out->xyUndist) out->xyUndist[2 * j] += 0.125f;
        if (out->angle) out->angle[j] = 30.0f * (float)j;
        if (out->response) out->response[j] = 10.0f - (float)j;
        if (out->octave) out->octave[j] = j % 3;
    }
    fillRows(desc, k);
    *nout = k;
    return PS_OK;
}
int ps_track_vo_pair(PsContext *ctx, const uint8_t *prevImg, const uint8_t *nextImg, const uint16_t *depth, int rows, int cols, int channels,
                     size_t rowStride, size_t depthStep, const PsKltParams *klt, const PsTrackVoParams *tp, const PsRansacParams *params,
                     const PsRansacConfig *cfg, const PsFrameGeometry *geometry, const PsTrackVoIn *in, int n, const PsTrackVoOut *out, int *numKept)
{
    Line("ps_track_vo_pair").a("ctx", ptr(ctx)).a("prevImg", image(prevImg, rows, cols, channels, rowStride, 1))
        .a("nextImg", image(nextImg, rows, cols, channels, rowStride, 1)).a("depth", image(depth, rows, cols, 1, depthStep, 2)).a("rows", rows)
        .a("cols", cols).a("channels", channels).a("rowStride", rowStride).a("depthStep", depthStep).a("klt", str(klt)).a("tp", str(tp))
        .a("params", str(params)).a("cfg", str(cfg)).a("geometry", str(geometry)).a("in.pairs", ptr(in->pairs)).a("in.depthFrame", ptr(in->depthFrame))
        .a("in.prevXY", arr(in->prevXY, n, 8)).a("in.prevPts", arr(in->prevPts, n, 12)).a("in.prevCounts", ptr(in->prevCounts))
        .a("in.prev", arr(&in->prev, 1, sizeof in->prev)).a("out.nextPts", arr(out->nextPts, n, 8)).a("out.status", ptr(out->status))
        .a("out.err", ptr(out->err)).a("out.matches", ptr(out->matches)).a("out.numMatches", ptr(out->numMatches)).a("out.keptIdx", ptr(out->keptIdx))
        .a("out.rows.xy", ptr(out->rows.xy)).a("out.rows.xyUndist", ptr(out->rows.xyUndist)).a("out.rows.pts", ptr(out->rows.pts))
        .a("out.rows.counts", ptr(out->rows.counts)).a("out.rows.angle", ptr(out->rows.angle)).a("out.rows.response", ptr(out->rows.response))
        .a("out.rows.octave", ptr(out->rows.octave)).a("out.rows.detDist", ptr(out->rows.detDist)).a("out.inlierMask", ptr(out->inlierMask))
        .a("out.pose", ptr(out->pose)).a("out.stats", ptr(out->stats)).a("numKept", ptr(numKept));
    if (int rc = failing("ps_track_vo_pair")) return rc;
    const int k = evens(n);
    int inl = 0;
    for (int j = 0; j < k; ++j) {
        out->keptIdx[j] = 2 * j;
        fillXY(out->rows.xy, j);
        fillXY(out->rows.xyUndist, j);
        out->rows.xyUndist[2 * j] += 0.125f;
        fillPts(out->rows.pts, j);
        out->matches[j] = dm(2 * j, j, 0.0f);
        out->inlierMask[j] = (uint8_t)(j % 2 == 0);
        inl += out->inlierMask[j];
    }
    fillPose(out->pose, (float)n);
    fillStats(out->stats, k, inl);
    *numKept = k;
    return PS_OK;
}
int ps_track_close_pair(PsContext *ctx, const uint8_t *img, const uint16_t *depth, int rows, int cols, int channels, size_t rowStride, size_t depthStep,
                        const PsFrontEndParams *params, const int8_t *pattern1024, const PsFrameGeometry *geometry, const PsTrackCloseParams *tp,
                        const PsTrackedRows *tracked, int n, uint8_t *desc, const PsTrackedRows *out, int32_t *srcIdx, int cap, int *nout, int *refill)
{
    Line("ps_track_close_pair").a("ctx", ptr(ctx)).a("img", image(img, rows, cols, channels, rowStride, 1))
        .a("depth", image(depth, rows, cols, 1, depthStep, 2)).a("rows", rows).a("cols", cols).a("channels", channels).a("rowStride", rowStride)
        .a("depthStep", depthStep).a("params", str(params)).a("pattern1024", ptr(pattern1024)).a("geometry", str(geometry)).a("tp", str(tp))
        .a("tracked.xy", arr(tracked->xy, n, 8)).a("tracked.xyUndist", arr(tracked->xyUndist, n, 8)).a("tracked.pts", arr(tracked->pts, n, 12))
        .a("tracked.counts", ptr(tracked->counts)).a("tracked.angle", arr(tracked->angle, n, 4)).a("tracked.response", arr(tracked->response, n, 4))
        .a("tracked.octave", arr(tracked->octave, n, 4)).a("tracked.detDist", arr(tracked->detDist, n, 8)).a("desc", ptr(desc))
        .a("out.xy", ptr(out->xy)).a("out.xyUndist", ptr(out->xyUndist)).a("out.pts", ptr(out->pts)).a("out.counts", ptr(out->counts))
        .a("out.angle", ptr(out->angle)).a("out.response", ptr(out->response)).a("out.octave", ptr(out->octave)).a("out.detDist", ptr(out->detDist))
        .a("srcIdx", ptr(srcIdx)).a("cap", cap).a("nout", ptr(nout)).a("refill", ptr(refill));
    if (int rc = failing("ps_track_close_pair")) return rc;
    const int k = cap < n + 2 ? cap : n + 2; // the tracked rows, then two merged ones
    for (int j = 0; j < k; ++j) {
        srcIdx[j] = j;
        fillXY(out->xy, j);
        fillXY(out->xyUndist, j);
        out->xyUndist[2 * j] += 0.125f;
        fillPts(out->pts, j);
        out->angle[j] = 30.0f * (float)j;
        out->response[j] = 10.0f - (float)j;
        out->octave[j] = j % 3;
        out->detDist[j] = 1.0 + (double)j;
    }
    fillRows(desc, k);
    *nout = k;
    *refill = 1;
    return PS_OK;
}

} // extern "C"
