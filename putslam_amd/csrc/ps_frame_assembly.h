// ps_frame_assembly.h -- from key points to a frame set without a host step (include/putslam_hip.h: "Frame assembly"): the gather
// of DBScan's survivors, the undistortion and back-projection of the described key points in the described order with the
// detection distances, and the PsFrontEnd handle that runs detect, thin, gather, pyramid build, describe and assemble on one stream.
// Part of the device translation unit (ps_capi.hip), after ps_dbscan.h, ps_orb.h and ps_orb_detect.h, whose launches it queues.
// Both kernels: one thread per output row, a grid of row blocks x frames, no LDS; the arithmetic is ps_geometry.h's undistort_point,
// depth_rule_offset and point_from_depth, stated there once.
#pragma once
#include "ps_geometry.h" // DistArgs, undistort_point, depth_rule_offset, depth_pixel, point_from_depth

namespace psdev {

// what ps_assemble_rows needs beside its arrays
struct AssembleArgs {
    DistArgs dist;
    double scale;
    const uint8_t *depth;                // frame 0 of the set
    size_t rowStride, frameStride, view; // resolved (depth_set_strides); `view`: what a frame spans, row padding included
    int rows, cols, firstFrame, cap;
};

// The undistorted position q of the distorted p and its 3-D point in the depth frame at `frame` (null: no depth image, depth 0 --
// the keypoints2Dto3D result for no depth): ps_geometry.h's undistort_point, depth_rule_offset, depth_pixel and point_from_depth.
// point2Dto3D of q in one frame of a depth set (ps_uncertainty.h back-projects pixels with it too)
PS_D void back_project_in_frame(float2 q, float fx, float fy, float cx, float cy, double scale, const uint8_t *__restrict__ frame, size_t rowStride,
                                int rows, int cols, float &X, float &Y, float &Z)
{
    // the rule over the frame as the DENSE image the reference holds: u == cols in a row that is not the last is the next row's
    // first pixel whatever the row stride -- a set's padding is alignment, not a parent image, and is never read
    size_t off = 0;
    unsigned dv = 0;
    if (frame != nullptr && depth_rule_offset(q.x, q.y, rows, cols, (size_t)cols * 2, (size_t)rows * (size_t)cols * 2, off)) {
        const unsigned pixel = (unsigned)(off >> 1), r = pixel / (unsigned)cols, c = pixel - r * (unsigned)cols;
        dv = depth_pixel(frame + (size_t)r * rowStride + (size_t)c * 2);
    }
    point_from_depth(q.x, q.y, dv, fx, fy, cx, cy, scale, X, Y, Z);
}

PS_D void undistort_and_back_project(float2 p, const DistArgs &dist, double scale, const uint8_t *__restrict__ frame, size_t rowStride, int rows,
                                     int cols, float2 &q, float &X, float &Y, float &Z)
{
    undistort_point(p.x, p.y, dist, q.x, q.y);
    back_project_in_frame(q, dist.fx, dist.fy, dist.cx, dist.cy, scale, frame, rowStride, rows, cols, X, Y, Z);
}

// Output row j of frame f is input row idx[f][j], j < nidx[f]; a count outside 0 .. cap: -1 and nothing else; an index outside
// 0 .. cap-1: a zero row
__global__ __launch_bounds__(kBlock) void ps_gather_rows(const int32_t *__restrict__ idx, const int32_t *__restrict__ nidx, int cap,
                                                         const float2 *__restrict__ xyIn, const float *__restrict__ respIn,
                                                         const float *__restrict__ angIn, const int32_t *__restrict__ octIn,
                                                         float2 *__restrict__ xyOut, float *__restrict__ respOut, float *__restrict__ angOut,
                                                         int32_t *__restrict__ octOut, int32_t *__restrict__ countsOut)
{
    const int f = (int)blockIdx.y, j = (int)(blockIdx.x * kBlock + threadIdx.x);
    const int n = nidx[f];
    const bool ok = n >= 0 && n <= cap;
    if (j == 0) countsOut[f] = ok ? n : -1;
    if (!ok || j >= n) return;
    const size_t base = (size_t)f * (size_t)cap, to = base + (size_t)j;
    const int i = idx[to];
    const bool in = i >= 0 && i < cap;
    const size_t from = base + (size_t)(in ? i : 0);
    xyOut[to] = in ? xyIn[from] : make_float2(0.f, 0.f);
    if (respOut) respOut[to] = in ? respIn[from] : 0.f;
    if (angOut) angOut[to] = in ? angIn[from] : 0.f;
    if (octOut) octOut[to] = in ? octIn[from] : 0;
}

// Output row j of frame f from key point i = keptIdx[f][j]: the distorted position, the undistorted one, the 3-D point read from
// depth frame firstFrame + f, the detection distance and the key point's own columns
__global__ __launch_bounds__(kBlock) void ps_assemble_rows(AssembleArgs a, const float2 *__restrict__ xy, const int32_t *__restrict__ keptIdx,
                                                           const int32_t *__restrict__ numKept, PsFrameRowsOut o)
{
    const int f = (int)blockIdx.y, j = (int)(blockIdx.x * kBlock + threadIdx.x);
    const int n = numKept[f];
    const bool ok = n >= 0 && n <= a.cap;
    if (j == 0) o.nkpts[f] = ok ? n : 0;
    if (!ok || j >= n) return;
    const size_t base = (size_t)f * (size_t)a.cap, to = base + (size_t)j;
    const int i = keptIdx[to];
    const bool in = i >= 0 && i < a.cap;
    const size_t from = base + (size_t)(in ? i : 0);
    float2 p = make_float2(0.f, 0.f), q = p;
    float X = 0.f, Y = 0.f, Z = 0.f, dist = 0.f;
    if (in) {
        p = xy[from];
        undistort_and_back_project(p, a.dist, a.scale, a.depth + (size_t)(a.firstFrame + f) * a.frameStride, a.rowStride, a.rows, a.cols, q,
                                   X, Y, Z);
        // matcher.cpp:53-55: float products, float sums left to right, std::sqrt(float) -- ps_sqrt is the correctly rounded root
        // (__fsqrt_rn is not: without OCML's rounded operations HIP maps it to the native, one-ulp instruction)
        dist = ps_sqrt((X * X + Y * Y) + Z * Z);
    }
    o.pts[3 * to] = X;
    o.pts[3 * to + 1] = Y;
    o.pts[3 * to + 2] = Z;
    if (o.xy) reinterpret_cast<float2 *>(o.xy)[to] = p;
    if (o.xyUndist) reinterpret_cast<float2 *>(o.xyUndist)[to] = q;
    if (o.angle) o.angle[to] = in ? o.angleIn[from] : 0.f;
    if (o.response) o.response[to] = in ? o.responseIn[from] : 0.f;
    if (o.octave) o.octave[to] = in ? o.octaveIn[from] : 0;
    if (o.srcIdx) o.srcIdx[to] = in ? i : 0;
    if (o.detDist) o.detDist[to] = (double)dist;
}

} // namespace psdev

// Host side: the handle, the checks, the launches and the entry points
struct PsFrontEnd {
    int device = 0;
    int rows = 0, cols = 0, cn = 0, maxFrames = 0;
    int rowCap = 0, need = 0; // rows a frame of the handle's arrays holds; rows a frame can emit
    PsFrontEndParams params{};
    PsOrbDetector *det = nullptr;
    PsOrbPyramids *pyr = nullptr;
    char *block = nullptr;    // every array below
    float *xy0 = nullptr, *resp0 = nullptr, *ang0 = nullptr, *xy1 = nullptr, *resp1 = nullptr, *ang1 = nullptr; // detected | thinned
    int32_t *oct0 = nullptr, *cnt0 = nullptr, *oct1 = nullptr, *cnt1 = nullptr;
    int32_t *thinIdx = nullptr, *thinN = nullptr, *keptIdx = nullptr, *numKept = nullptr, *slots = nullptr;
};

namespace {

constexpr int kFrontEndMinPts = 2, kFrontEndFromCluster = 1; // DBScan's defaults (dbscan.h:19)

int rows_grid_check(PsContext *ctx, int F, int capacity, const char *who)
{
    if (F < 0 || F > kImageMaxFrames) return fail(ctx, PS_ERR_BAD_ARG, (std::string(who) + ": F outside 0 .. 65535").c_str());
    if (capacity > PS_MAX_KPTS) return fail(ctx, PS_ERR_UNSUPPORTED, (std::string(who) + ": capacity above PS_MAX_KPTS").c_str());
    if (capacity < 1) return fail(ctx, PS_ERR_BAD_ARG, (std::string(who) + ": capacity < 1").c_str());
    return PS_OK;
}

dim3 rows_grid(int F, int capacity) { return dim3((unsigned)((capacity + kBlock - 1) / kBlock), (unsigned)F); }

int gather_launch(PsContext *ctx, const int32_t *idx, const int32_t *nidx, int F, int cap, const float *xyIn, const float *responseIn,
                  const float *angleIn, const int32_t *octaveIn, float *xyOut, float *responseOut, float *angleOut, int32_t *octaveOut,
                  int32_t *countsOut)
{
    hipLaunchKernelGGL(ps_gather_rows, rows_grid(F, cap), dim3(kBlock), 0, ctx->stream, idx, nidx, cap, reinterpret_cast<const float2 *>(xyIn),
                       responseIn, angleIn, octaveIn, reinterpret_cast<float2 *>(xyOut), responseOut, angleOut, octaveOut, countsOut);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

// geometry, the depth set and the output block as the three calls take them; `a` resolved.  needCounts: out->nkpts is required (the
// host form returns its one count by *nout); sideInputs: the caller passes angleIn / responseIn / octaveIn (the front end puts
// its own there)
int assemble_check(PsContext *ctx, const PsFrameGeometry *g, const PsDepthSet *depth, int firstDepthFrame, int F, const PsFrameRowsOut *out,
                   bool needCounts, bool sideInputs, const char *who, AssembleArgs &a)
{
    const auto msg = [who](const char *what) { return std::string(who) + what; };
    if (!g || !depth || !out) return fail(ctx, PS_ERR_BAD_ARG, msg(": null geometry, depth set or output block").c_str());
    if (!out->pts || (needCounts && !out->nkpts)) return fail(ctx, PS_ERR_BAD_ARG, msg(": out->pts and out->nkpts are required").c_str());
    if (sideInputs && ((out->angle && !out->angleIn) || (out->response && !out->responseIn) || (out->octave && !out->octaveIn)))
        return fail(ctx, PS_ERR_BAD_ARG, msg(": angle, response or octave wanted without its input").c_str());
    if (!depth_set_strides(*depth, a.rowStride, a.frameStride, a.view))
        return fail(ctx, PS_ERR_BAD_ARG, msg(": depth set: rows and cols in 1 .. 8192, even strides, rowStride at least a row, frameStride at least a view").c_str());
    if (firstDepthFrame < 0 || depth->numFrames < 0 || (long long)firstDepthFrame + F > depth->numFrames)
        return fail(ctx, PS_ERR_BAD_ARG, msg(": depth frames outside the set").c_str());
    if (F > 0 && !depth->pixels) return fail(ctx, PS_ERR_BAD_ARG, msg(": null depth pixels").c_str());
    for (int i = 0; i < 5; ++i) a.dist.k[i] = g->dist5[i];
    a.dist.fx = g->K[0];
    a.dist.fy = g->K[4];
    a.dist.cx = g->K[2];
    a.dist.cy = g->K[5];
    a.scale = g->depthImageScale;
    a.depth = reinterpret_cast<const uint8_t *>(depth->pixels);
    a.rows = depth->rows;
    a.cols = depth->cols;
    a.firstFrame = firstDepthFrame;
    return PS_OK;
}

int assemble_launch(PsContext *ctx, AssembleArgs a, const float *xy, const int32_t *keptIdx, const int32_t *numKept, int F, int cap,
                    const PsFrameRowsOut &out)
{
    a.cap = cap;
    hipLaunchKernelGGL(ps_assemble_rows, rows_grid(F, cap), dim3(kBlock), 0, ctx->stream, a, reinterpret_cast<const float2 *>(xy), keptIdx, numKept,
                       out);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

// every launch of the front end for F frames whose rows lie `cap` apart; the arguments were checked
int front_end_launch(PsContext *ctx, PsFrontEnd *fe, const uint8_t *pixels, size_t row, size_t frame, int F, const AssembleArgs &a, int cap,
                     uint8_t *desc, PsFrameRowsOut out)
{
    const OrbDetPlan pl = orbdet_plan(fe->det, fe->params.detect);
    int rc = orbdet_launch(ctx, fe->det, pixels, row, frame, F, pl, cap, fe->xy0, fe->resp0, fe->ang0, fe->oct0, fe->cnt0, kOrbDetPassAll);
    if (rc) return rc;
    rc = dbscan_launch(ctx, fe->xy0, fe->oct0, fe->cnt0, 0, F, cap, fe->params.DBScanEps, kFrontEndMinPts, kFrontEndFromCluster, fe->thinIdx,
                       fe->thinN);
    if (rc) return rc;
    rc = gather_launch(ctx, fe->thinIdx, fe->thinN, F, cap, fe->xy0, fe->resp0, fe->ang0, fe->oct0, fe->xy1, fe->resp1, fe->ang1, fe->oct1,
                       fe->cnt1);
    if (rc) return rc;
    rc = orb_build_launch(ctx, fe->pyr, pixels, row, frame, F, 0, kOrbPassAll);
    if (rc) return rc;
    rc = orb_describe_launch(ctx, fe->pyr, fe->slots, fe->xy1, fe->ang1, fe->oct1, fe->cnt1, F, cap, desc, fe->keptIdx, fe->numKept, kOrbPassAll);
    if (rc) return rc;
    out.angleIn = fe->ang1;
    out.responseIn = fe->resp1;
    out.octaveIn = fe->oct1;
    return assemble_launch(ctx, a, fe->xy1, fe->keptIdx, fe->numKept, F, cap, out);
}

} // namespace

extern "C" {

size_t ps_abi_sizeof_depth_set(void) { return sizeof(PsDepthSet); }
size_t ps_abi_sizeof_frame_geometry(void) { return sizeof(PsFrameGeometry); }
size_t ps_abi_sizeof_frame_rows_out(void) { return sizeof(PsFrameRowsOut); }
size_t ps_abi_sizeof_front_end_params(void) { return sizeof(PsFrontEndParams); }

int ps_gather_keypoints(PsContext *ctx, const int32_t *idx, const int32_t *nidx, int F, int capacity, const float *xyIn,
                        const float *responseIn, const float *angleIn, const int32_t *octaveIn, float *xyOut, float *responseOut,
                        float *angleOut, int32_t *octaveOut, int32_t *countsOut)
{
    int rc = bind(ctx);
    if (rc) return rc;
    rc = rows_grid_check(ctx, F, capacity, "ps_gather_keypoints");
    if (rc) return rc;
    if (!responseIn != !responseOut || !angleIn != !angleOut || !octaveIn != !octaveOut)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_gather_keypoints: response, angle and octave are In / Out pairs: both or neither");
    if (F == 0) return PS_OK;
    if (!idx || !nidx || !xyIn || !xyOut || !countsOut) return fail(ctx, PS_ERR_BAD_ARG, "ps_gather_keypoints: null array");
    TimingOff toff(ctx);
    HandoffGuard handoffGuard{ctx};
    return gather_launch(ctx, idx, nidx, F, capacity, xyIn, responseIn, angleIn, octaveIn, xyOut, responseOut, angleOut, octaveOut, countsOut);
}

int ps_assemble_frames(PsContext *ctx, const PsFrameGeometry *geometry, const PsDepthSet *depth, int firstDepthFrame, const float *xy,
                       const int32_t *keptIdx, const int32_t *numKept, int F, int capacity, const PsFrameRowsOut *out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    rc = rows_grid_check(ctx, F, capacity, "ps_assemble_frames");
    if (rc) return rc;
    AssembleArgs a{};
    rc = assemble_check(ctx, geometry, depth, firstDepthFrame, F, out, true, true, "ps_assemble_frames", a);
    if (rc) return rc;
    if (F == 0) return PS_OK;
    if (!xy || !keptIdx || !numKept) return fail(ctx, PS_ERR_BAD_ARG, "ps_assemble_frames: null array");
    TimingOff toff(ctx);
    HandoffGuard handoffGuard{ctx};
    return assemble_launch(ctx, a, xy, keptIdx, numKept, F, capacity, *out);
}

int ps_front_end_create(PsContext *ctx, int rows, int cols, int channels, const PsFrontEndParams *params, const int8_t *pattern1024,
                        int maxFrames, PsFrontEnd **out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!out) return fail(ctx, PS_ERR_BAD_ARG, "ps_front_end_create: null out");
    *out = nullptr;
    if (!params) return fail(ctx, PS_ERR_BAD_ARG, "ps_front_end_create: null PsFrontEndParams");
    rc = orbdet_params_check(ctx, &params->detect);
    if (rc) return rc;
    if (const char *why = orb_params_error(&params->describe)) return fail(ctx, PS_ERR_BAD_ARG, why);
    if (params->detect.maximalTrackedFeatures > PS_DBSCAN_MAX_KPTS)
        return fail(ctx, PS_ERR_UNSUPPORTED, "ps_front_end_create: maximalTrackedFeatures above PS_DBSCAN_MAX_KPTS");
    HandleOwner<PsFrontEnd> own(new PsFrontEnd, ps_front_end_destroy);
    PsFrontEnd *fe = own.get();
    fe->device = ctx->device;
    fe->rows = rows;
    fe->cols = cols;
    fe->cn = channels;
    fe->maxFrames = maxFrames;
    fe->params = *params;
    rc = ps_orb_detector_create(ctx, rows, cols, channels, &params->detect, maxFrames, &fe->det); // (shape and maxFrames: checked there)
    if (rc) return rc;
    rc = ps_orb_pyramids_create(ctx, rows, cols, channels, &params->describe, pattern1024, maxFrames, &fe->pyr);
    if (rc) return rc;
    const OrbDetPlan pl = orbdet_plan(fe->det, params->detect);
    if (pl.any()) { // the ROI lists a frames call would otherwise allocate at its first use
        rc = orbdet_reserve(ctx, fe->det, pl);
        if (rc) return rc;
    }
    fe->need = (int)pl.need;
    fe->rowCap = params->detect.maximalTrackedFeatures > 1 ? params->detect.maximalTrackedFeatures : 1;
    const size_t Fm = (size_t)maxFrames, N = Fm * (size_t)fe->rowCap;
    BlockLayout lay;
    const size_t oXy0 = lay.take<float2>(N, 16), oResp0 = lay.take<float>(N, 16), oAng0 = lay.take<float>(N, 16), oOct0 = lay.take<int32_t>(N, 16),
                 oXy1 = lay.take<float2>(N, 16), oResp1 = lay.take<float>(N, 16), oAng1 = lay.take<float>(N, 16), oOct1 = lay.take<int32_t>(N, 16),
                 oThin = lay.take<int32_t>(N, 16), oKept = lay.take<int32_t>(N, 16), oCnt0 = lay.take<int32_t>(Fm, 16),
                 oCnt1 = lay.take<int32_t>(Fm, 16), oThinN = lay.take<int32_t>(Fm, 16), oNumKept = lay.take<int32_t>(Fm, 16),
                 oSlots = lay.take<int32_t>(Fm, 16);
    std::vector<int32_t> ident(Fm);
    for (size_t f = 0; f < Fm; ++f) ident[f] = (int32_t)f; // frame f is described in slot f
    hipError_t e = hipMalloc((void **)&fe->block, lay.total);
    if (e == hipSuccess) e = hipMemset(fe->block, 0, lay.total);
    if (e == hipSuccess) e = hipMemcpy(fe->block + oSlots, ident.data(), Fm * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(ctx, PS_ERR_ALLOC, "ps_front_end_create: hipMalloc", e);
    char *b = fe->block;
    fe->xy0 = (float *)(b + oXy0), fe->resp0 = (float *)(b + oResp0), fe->ang0 = (float *)(b + oAng0), fe->oct0 = (int32_t *)(b + oOct0);
    fe->xy1 = (float *)(b + oXy1), fe->resp1 = (float *)(b + oResp1), fe->ang1 = (float *)(b + oAng1), fe->oct1 = (int32_t *)(b + oOct1);
    fe->thinIdx = (int32_t *)(b + oThin), fe->keptIdx = (int32_t *)(b + oKept), fe->cnt0 = (int32_t *)(b + oCnt0), fe->cnt1 = (int32_t *)(b + oCnt1);
    fe->thinN = (int32_t *)(b + oThinN), fe->numKept = (int32_t *)(b + oNumKept), fe->slots = (int32_t *)(b + oSlots);
    *out = own.release();
    return PS_OK;
}

void ps_front_end_destroy(PsFrontEnd *fe)
{
    if (!fe) return;
    (void)hipSetDevice(fe->device);
    if (fe->block) (void)hipFree(fe->block); // (hipFree waits for the device: queued work that reads the handle has finished)
    ps_orb_detector_destroy(fe->det);
    ps_orb_pyramids_destroy(fe->pyr);
    delete fe;
}

int ps_front_end_frames(PsContext *ctx, PsFrontEnd *fe, const PsImageSet *images, const PsDepthSet *depth, const PsFrameGeometry *geometry,
                        int capacity, uint8_t *desc, const PsFrameRowsOut *out)
{
    static const char *who = "ps_front_end_frames";
    int rc = bind(ctx);
    if (rc) return rc;
    if (capacity > PS_DBSCAN_MAX_KPTS) return fail(ctx, PS_ERR_UNSUPPORTED, "ps_front_end_frames: capacity above PS_DBSCAN_MAX_KPTS");
    size_t row = 0, frame = 0;
    rc = check_image_set(ctx, fe, &PsFrontEnd::maxFrames, images, 0, who, row, frame);
    if (rc) return rc;
    AssembleArgs a{};
    rc = assemble_check(ctx, geometry, depth, 0, images->numFrames, out, true, false, who, a);
    if (rc) return rc;
    if (depth->numFrames != images->numFrames || depth->rows != fe->rows || depth->cols != fe->cols)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_front_end_frames: the depth set's numFrames, rows and cols must be the images'");
    if (capacity < 1 || capacity < fe->need || capacity > fe->rowCap)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_front_end_frames: capacity must hold what a frame can emit and not exceed max(1, maximalTrackedFeatures)");
    if (images->numFrames == 0) return PS_OK;
    if (!desc) return fail(ctx, PS_ERR_BAD_ARG, "ps_front_end_frames: null desc");
    TimingOff toff(ctx);
    HandoffGuard handoffGuard{ctx};
    return front_end_launch(ctx, fe, images->pixels, row, frame, images->numFrames, a, capacity, desc, *out);
}

int ps_front_end_frame(PsContext *ctx, const uint8_t *img, const uint16_t *depth, int rows, int cols, int channels, size_t rowStride,
                       size_t depthStep, const PsFrontEndParams *params, const int8_t *pattern1024, const PsFrameGeometry *geometry,
                       uint8_t *desc, const PsFrameRowsOut *out, int cap, int *nout)
{
    static const char *who = "ps_front_end_frame";
    int rc = bind(ctx);
    if (rc) return rc;
    rc = image_shape_error(ctx, rows, cols, channels, who);
    if (rc) return rc;
    rowStride = image_row_stride(cols, channels, rowStride);
    if (!img || !depth || !nout || rowStride == 0 || cap < 0 || (cap > 0 && !desc))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_front_end_frame: null array, negative cap or a row stride below a row");
    PsDepthSet ds{};
    ds.rowStride = depthStep;
    ds.numFrames = 1;
    ds.rows = rows;
    ds.cols = cols;
    AssembleArgs a{};
    ds.pixels = depth; // (the host array: checked for NULL only; the device copy is named below)
    rc = assemble_check(ctx, geometry, &ds, 0, 1, out, false, false, who, a);
    if (rc) return rc;
    TimingOff toff(ctx);
    PsFrontEnd *fe = nullptr;
    rc = ps_front_end_create(ctx, rows, cols, channels, params, pattern1024, 1, &fe);
    if (rc) return rc;
    const HandleOwner<PsFrontEnd> own(fe, ps_front_end_destroy);
    const size_t room = (size_t)(fe->need > 1 ? fe->need : 1), imgBytes = image_bytes(rows, cols, channels, rowStride);
    // one block: the image | the depth view | nkpts | pts | xy | xyUndist | angle | response | octave | srcIdx | detDist | desc
    BlockLayout lay;
    lay.take<uint8_t>(imgBytes);
    const size_t oDepth = lay.take<uint16_t>(a.view / 2, 16), oN = lay.take<int32_t>(1, 16), oPts = lay.take<float>(3 * room),
                 oXy = lay.take<float2>(room), oUn = lay.take<float2>(room), oAng = lay.take<float>(room), oResp = lay.take<float>(room),
                 oOct = lay.take<int32_t>(room), oSrc = lay.take<int32_t>(room), oDist = lay.take<double>(room),
                 oDesc = lay.take<uint8_t>(room * 32, 16), total = lay.total;
    const DeviceBlock blk(total);
    if (blk.err != hipSuccess) return fail(ctx, PS_ERR_ALLOC, "hipMalloc", blk.err);
    char *d = blk.p;
    PS_HIP(hipMemcpyAsync(d, img, imgBytes, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpyAsync(d + oDepth, depth, a.view, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream)); // (pageable sources may change)
    a.depth = (const uint8_t *)(d + oDepth);
    PsFrameRowsOut dev{};
    dev.pts = (float *)(d + oPts);
    dev.nkpts = (int32_t *)(d + oN);
    dev.xy = (float *)(d + oXy);
    dev.xyUndist = (float *)(d + oUn);
    dev.angle = (float *)(d + oAng);
    dev.response = (float *)(d + oResp);
    dev.octave = (int32_t *)(d + oOct);
    dev.srcIdx = (int32_t *)(d + oSrc);
    dev.detDist = (double *)(d + oDist);
    rc = front_end_launch(ctx, fe, (const uint8_t *)d, rowStride, 0, 1, a, (int)room, (uint8_t *)(d + oDesc), dev);
    if (rc) return rc;
    std::vector<char> back(total - oN);
    PS_HIP(hipMemcpyAsync(back.data(), d + oN, back.size(), hipMemcpyDeviceToHost, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream));
    int32_t n = 0;
    std::memcpy(&n, back.data(), 4);
    if (n < 0 || (size_t)n > room) return fail(ctx, PS_ERR_HIP, "ps_front_end_frame: the device returned an impossible count");
    *nout = n;
    if (n > cap) return fail(ctx, PS_ERR_BAD_ARG, "ps_front_end_frame: cap is too small (*nout = required)");
    const size_t k = (size_t)n;
    const auto take = [&](void *to, size_t off, size_t bytes) { if (to && k > 0) std::memcpy(to, back.data() + (off - oN), k * bytes); };
    take(out->pts, oPts, 12);
    take(out->xy, oXy, 8);
    take(out->xyUndist, oUn, 8);
    take(out->angle, oAng, 4);
    take(out->response, oResp, 4);
    take(out->octave, oOct, 4);
    take(out->srcIdx, oSrc, 4);
    take(out->detDist, oDist, 8);
    take(desc, oDesc, 32);
    return PS_OK;
}

} // extern "C"
