// putslam_dropin_patches.cpp -- the drop-in's MatchingOnPatches (putslam_dropin.h): the reference's three
// calls over ps_compute_patch / ps_compute_patch_gradient / ps_optimize_location and the batch form over ps_optimize_locations.  A
// translation unit of its own beside putslam_dropin.cpp, whose calling thread's context it uses.
#include "putslam_dropin.h"

#include <cmath>
#include <iostream>
#include <limits>

#include "putslam_hip.h"

namespace putslam_hip {
PsContext *dropinThreadContext(int *status);
void dropinReportError(const PsContext *ctx);
} // namespace putslam_hip

namespace {

thread_local int lastStatus_ = PS_PATCH_MAX_ITERATIONS, lastIterations_ = 0;

PsPatchParams paramsOf(const MatchingOnPatches::parameters &p)
{
    PsPatchParams q{};
    q.minSqrtIncrement = p.minSqrtIncrement;
    q.patchSize = p.patchSize;
    q.maxIter = p.maxIter;
    return q;
}

// an 8-bit image of one or three channels, as assertGrayscale takes it
bool imageOk(const cv::Mat &img, const char *who)
{
    if (!img.empty() && img.depth() == CV_8U && (img.channels() == 1 || img.channels() == 3)) return true;
    std::cerr << "putslam_hip: " << who << ": the image must be CV_8UC1 or CV_8UC3 and not empty" << std::endl;
    return false;
}

// rows x cols x channels bytes with dense rows: what two images of different steps are brought to
std::vector<unsigned char> denseCopy(const cv::Mat &img)
{
    const size_t row = (size_t)img.cols * img.channels();
    std::vector<unsigned char> out(row * (size_t)img.rows);
    for (int r = 0; r < img.rows; ++r) std::memcpy(out.data() + (size_t)r * row, img.data + (size_t)r * img.step, row);
    return out;
}

void fillNaN(Eigen::Matrix3f &m)
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) m(i, j) = std::numeric_limits<float>::quiet_NaN();
}

} // namespace

// One place fills the block: the half size is derived, warping is never on (the reference parses it and reads it nowhere)
MatchingOnPatches::MatchingOnPatches(int size, int stepLimit, double threshold, int verbosity)
    : params{verbosity, false, size, (size - 1) / 2, stepLimit, threshold}
{
}

MatchingOnPatches::MatchingOnPatches(parameters block) : MatchingOnPatches(block.patchSize, block.maxIter, block.minSqrtIncrement, block.verbose) {}

int MatchingOnPatches::lastStatus() { return lastStatus_; }
int MatchingOnPatches::lastIterations() { return lastIterations_; }

std::vector<double> MatchingOnPatches::computePatch(cv::Mat img, double x, double y)
{
    std::vector<double> none;
    if (!imageOk(img, "computePatch")) return none;
    int status;
    PsContext *ctx = putslam_hip::dropinThreadContext(&status);
    if (!ctx) return none;
    const PsPatchParams prm = paramsOf(params);
    const double pt[2] = {x, y};
    std::vector<double> patch((size_t)params.patchSize * (size_t)(params.patchSize > 0 ? params.patchSize : 0));
    uint8_t st = 0;
    status = ps_compute_patch(ctx, img.data, img.rows, img.cols, img.channels(), (size_t)img.step, pt, 1, &prm, patch.data(), &st);
    if (status != PS_OK) {
        putslam_hip::dropinReportError(ctx);
        return none;
    }
    if (st == PS_PATCH_OLD_TAPS_OUTSIDE) {
        std::cerr << "putslam_hip: computePatch: the patch's taps leave the image at (" << x << ", " << y << ")" << std::endl;
        return none;
    }
    return patch;
}

void MatchingOnPatches::computeGradient(cv::Mat img, double x, double y, Eigen::Matrix3f &InvHessian, std::vector<float> &gradientX,
                                        std::vector<float> &gradientY)
{
    fillNaN(InvHessian);
    if (!imageOk(img, "computeGradient")) return;
    int status;
    PsContext *ctx = putslam_hip::dropinThreadContext(&status);
    if (!ctx) return;
    const PsPatchParams prm = paramsOf(params);
    const double pt[2] = {x, y};
    const size_t E = (size_t)params.patchSize * (size_t)(params.patchSize > 0 ? params.patchSize : 0);
    std::vector<float> gx(E), gy(E);
    float inv[9];
    uint8_t st = 0;
    status = ps_compute_patch_gradient(ctx, img.data, img.rows, img.cols, img.channels(), (size_t)img.step, pt, 1, &prm, gx.data(), gy.data(), inv,
                                       &st);
    if (status != PS_OK) {
        putslam_hip::dropinReportError(ctx);
        return;
    }
    if (st == PS_PATCH_OLD_TAPS_OUTSIDE) {
        std::cerr << "putslam_hip: computeGradient: the patch's taps leave the image at (" << x << ", " << y << ")" << std::endl;
        return;
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) InvHessian(i, j) = inv[3 * i + j];
    gradientX.insert(gradientX.end(), gx.begin(), gx.end()); // (the reference push_backs)
    gradientY.insert(gradientY.end(), gy.begin(), gy.end());
}

bool MatchingOnPatches::optimizeLocation(cv::Mat oldImg, std::vector<double> oldPatch, cv::Mat newImg, double &newX, double &newY,
                                         std::vector<float> gradientX, std::vector<float> gradientY, Eigen::Matrix3f &InvHessian)
{
    lastIterations_ = 0;
    if (std::isnan(InvHessian(0, 0))) { // (:108, before anything else)
        lastStatus_ = PS_PATCH_NAN_HESSIAN;
        return false;
    }
    lastStatus_ = PS_PATCH_OLD_TAPS_OUTSIDE;
    if (!imageOk(newImg, "optimizeLocation")) return false;
    const size_t E = (size_t)params.patchSize * (size_t)(params.patchSize > 0 ? params.patchSize : 0);
    if (oldPatch.size() != E || gradientX.size() != E || gradientY.size() != E) {
        std::cerr << "putslam_hip: optimizeLocation: the patch and the gradients must hold patchSize x patchSize elements" << std::endl;
        return false;
    }
    int status;
    PsContext *ctx = putslam_hip::dropinThreadContext(&status);
    if (!ctx) return false;
    const PsPatchParams prm = paramsOf(params);
    float inv[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) inv[3 * i + j] = InvHessian(i, j);
    double pt[2] = {newX, newY};
    uint8_t st = 0;
    int32_t it = 0;
    status = ps_optimize_location(ctx, oldImg.data, oldPatch.data(), newImg.data, newImg.rows, newImg.cols, newImg.channels(), (size_t)newImg.step,
                                  pt, 1, gradientX.data(), gradientY.data(), inv, &prm, &st, &it);
    if (status != PS_OK) {
        putslam_hip::dropinReportError(ctx);
        return false;
    }
    newX = pt[0];
    newY = pt[1];
    lastStatus_ = st;
    lastIterations_ = it;
    return st == PS_PATCH_CONVERGED;
}

std::vector<int> MatchingOnPatches::optimizeLocations(cv::Mat oldImg, cv::Mat newImg, const std::vector<double> &oldXY, std::vector<double> &newXY,
                                                      std::vector<int> *iterations)
{
    std::vector<int> none;
    if (iterations) iterations->clear();
    if (!imageOk(oldImg, "optimizeLocations") || !imageOk(newImg, "optimizeLocations")) return none;
    if (oldImg.rows != newImg.rows || oldImg.cols != newImg.cols || oldImg.channels() != newImg.channels() || oldXY.size() != newXY.size() ||
        (oldXY.size() & 1) != 0) {
        std::cerr << "putslam_hip: optimizeLocations: two images of one shape and two lists of as many x, y pairs" << std::endl;
        return none;
    }
    const int n = (int)(oldXY.size() / 2);
    if (n == 0) return none;
    int status;
    PsContext *ctx = putslam_hip::dropinThreadContext(&status);
    if (!ctx) return none;
    const PsPatchParams prm = paramsOf(params);
    std::vector<unsigned char> denseOld, denseNew; // (the call takes one row stride for both images)
    const unsigned char *po = oldImg.data, *pn = newImg.data;
    size_t step = (size_t)oldImg.step;
    if (oldImg.step != newImg.step) {
        denseOld = denseCopy(oldImg);
        denseNew = denseCopy(newImg);
        po = denseOld.data(), pn = denseNew.data();
        step = 0;
    }
    std::vector<uint8_t> st((size_t)n);
    std::vector<int32_t> it((size_t)n);
    std::vector<double> xy = newXY;
    status = ps_optimize_locations(ctx, po, pn, oldImg.rows, oldImg.cols, oldImg.channels(), step, oldXY.data(), xy.data(), n, &prm, st.data(),
                                   it.data());
    if (status != PS_OK) {
        putslam_hip::dropinReportError(ctx);
        return none;
    }
    newXY = xy;
    if (iterations) iterations->assign(it.begin(), it.end());
    return std::vector<int>(st.begin(), st.end());
}
