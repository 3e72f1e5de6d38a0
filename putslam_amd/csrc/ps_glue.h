// ps_glue.h -- what the entry points of the device translation unit share on the HOST side, each rule once: the guard that marks
// queued work for a later ps_context_set_stream, the timing record's prologue and its switch, the PsFrameSet stride rule, the
// bisection behind the host-found bounds, and the image front end's guards and checks.  Host code only; included by ps_capi.hip and by the feature headers' host parts.
#pragma once
#include <climits>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>

#include "ps_image_rule.h"
#include "ps_internal.h"

namespace {

// An asynchronous call returns with its work still queued.  Whatever happens after the first launch -- success or an error half
// way (an allocation failure for a later block, a launch failure) -- the end of what WAS queued is marked for a later
// ps_context_set_stream: the new stream must not touch the shared arena before that work has finished.  The guard stands
// before the first thing the call may queue (prepare_score may already queue a clearing).
struct HandoffGuard {
    PsContext *c;
    ~HandoffGuard()
    {
        if (!c->handoff && hipEventCreateWithFlags(&c->handoff, hipEventDisableTiming) != hipSuccess) {
            c->handoff = nullptr;
            (void)hipStreamSynchronize(c->stream); // no event to wait on: drain instead
            return;
        }
        if (hipEventRecord(c->handoff, c->stream) == hipSuccess)
            c->handoffPending = true;
        else
            (void)hipStreamSynchronize(c->stream);
    }
};

// The host-pointer entry points are not part of the timed record.
struct TimingOff {
    PsContext *c;
    bool saved;
    explicit TimingOff(PsContext *ctx) : c(ctx), saved(ctx->timing) { c->timing = false; }
    ~TimingOff() { c->timing = saved; }
};

// A timed call (the VO and the map batch) takes the next slot of the timing ring; tick() records into it.
inline void begin_timed_call(PsContext *ctx)
{
    if (!ctx->timing) return;
    ctx->curCall = (int)(ctx->timedCalls++ % kTimingRing);
    ctx->slotMask[ctx->curCall] = 0;
}

void tick(PsContext *ctx, int slot, bool stop)
{
    if (!ctx->timing || slot >= kMaxTimed || ctx->ev.empty()) return;
    (void)hipEventRecord(ctx->ev[((size_t)ctx->curCall * kMaxTimed + slot) * 2 + (stop ? 1 : 0)], ctx->stream);
    if (stop) {
        ctx->slotMask[ctx->curCall] |= 1u << slot;
        if (slot + 1 > ctx->nTimed) ctx->nTimed = slot + 1;
    }
}

void identity16(float *T)
{
    for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.0f : 0.0f;
}

// Bytes between consecutive frames of a PsFrameSet, resolved, and the same in the units the kernels index with.
struct FrameStrides {
    size_t desc = 0, pts = 0;
    int descDwords() const { return (int)(desc / 4); }
    int descUint4() const { return (int)(desc / 16); }
    int ptsFloats() const { return (int)(pts / 4); }
};

// THE STRIDE RULE of a PsFrameSet (include/putslam_hip.h), for a set whose maxKpts is at least 1: a stride of 0 means dense;
// descFrameStride is a multiple of 16 and at least maxKpts x 32, desc itself 16-byte aligned; ptsFrameStride is a multiple of 4
// and at least maxKpts x 12; either divided by 4 fits an int (the kernels' index type).  needDesc / needPts = false: the call
// reads no descriptors / no points, and that half of the set is not looked at (its resolved stride is still returned).
// Returns PS_ERR_BAD_ARG with `who` in the message.
inline int frame_strides(PsContext *ctx, const PsFrameSet &fs, bool needDesc, bool needPts, const char *who, FrameStrides &out)
{
    const size_t denseDesc = (size_t)fs.maxKpts * 32, densePts = (size_t)fs.maxKpts * 12;
    out.desc = fs.descFrameStride ? fs.descFrameStride : denseDesc;
    out.pts = fs.ptsFrameStride ? fs.ptsFrameStride : densePts;
    if (needDesc && ((out.desc & 15) != 0 || out.desc < denseDesc || out.desc / 4 > (size_t)INT_MAX || ((uintptr_t)fs.desc & 15) != 0))
        return fail(ctx, PS_ERR_BAD_ARG, (std::string(who) + ": descFrameStride must be a multiple of 16, >= maxKpts x 32 and below 8 GiB, "
                                                             "desc 16-byte aligned").c_str());
    if (needPts && ((out.pts & 3) != 0 || out.pts < densePts || out.pts / 4 > (size_t)INT_MAX))
        return fail(ctx, PS_ERR_BAD_ARG, (std::string(who) + ": ptsFrameStride must be a multiple of 4, >= maxKpts x 12 and below 8 GiB").c_str());
    return PS_OK;
}

// A complete set as the map calls take it (views, frames, the views a call writes): every array, at least one frame, 1 ..
// PS_MAX_KPTS keypoints a frame, and the stride rule.
inline int check_frame_set(PsContext *ctx, const PsFrameSet &fs, const char *who, FrameStrides &out)
{
    if (!fs.desc || !fs.pts || !fs.nkpts || fs.maxKpts < 1 || fs.numFrames < 1)
        return fail(ctx, PS_ERR_BAD_ARG, (std::string(who) + ": bad frame set (null array, maxKpts or numFrames < 1)").c_str());
    if (fs.maxKpts > PS_MAX_KPTS)
        return fail(ctx, PS_ERR_UNSUPPORTED, (std::string(who) + ": more than PS_MAX_KPTS keypoints per view / frame").c_str());
    return frame_strides(ctx, fs, true, true, who, out);
}

// (depth_view_bytes, the addressable bytes of a 16-bit depth image, stands in ps_image_rule.h with the PsDepthSet rule)

// ---- the image front end (ps_klt.h, ps_fast.h, ps_orb.h); the arithmetic is ps_image_rule.h's ----

// The device block of a host form: allocated here (err says how that went), freed at every exit.
struct DeviceBlock {
    char *p = nullptr;
    const hipError_t err;
    explicit DeviceBlock(size_t bytes) : err(hipMalloc((void **)&p, bytes)) {}
    ~DeviceBlock() { if (p) (void)hipFree(p); }
};

// A handle (a pyramid set, a detector) with its destroy function: destroyed at every exit unless it was released.
template <class T> using HandleOwner = std::unique_ptr<T, void (*)(T *)>;

// The shape of an image as every front-end call takes it (KLT has its window rules in front of this one).
inline int image_shape_error(PsContext *ctx, int rows, int cols, int channels, const char *who)
{
    if (rows < 1 || cols < 1 || (channels != 1 && channels != 3))
        return fail(ctx, PS_ERR_BAD_ARG, (std::string(who) + ": rows and cols at least 1, channels 1 or 3").c_str());
    if (rows > kImageMaxDim || cols > kImageMaxDim)
        return fail(ctx, PS_ERR_UNSUPPORTED, (std::string(who) + ": image above 8192 rows or columns").c_str());
    return PS_OK;
}

// THE IMAGE-SET RULE, for an owner (device, rows, cols, cn; `slots` names its slot count) that takes the set's frames into slots
// firstSlot ..: owner and set are there, the owner is this device's, the frames are not negative and fit into the slots, the
// shape is the owner's, the strides resolve (image_set_strides; returned) and, with frames, there are pixels.  pixels = false
// leaves the last to the caller (ps_detect_features_device looks at it after its capacity rules).
template <class Owner>
int check_image_set(PsContext *ctx, const Owner *own, int Owner::*slots, const PsImageSet *images, int firstSlot, const char *who, size_t &row,
                    size_t &frame, bool pixels = true)
{
    if (!own || !images || own->device != ctx->device || images->numFrames < 0 || firstSlot < 0 ||
        (long long)firstSlot + images->numFrames > own->*slots)
        return fail(ctx, PS_ERR_BAD_ARG, (std::string(who) + ": null argument, another device's handle, or slots outside the set").c_str());
    if (images->rows != own->rows || images->cols != own->cols || images->channels != own->cn || !image_set_strides(*images, row, frame))
        return fail(ctx, PS_ERR_BAD_ARG, (std::string(who) + ": the images' shape differs from the handle's, or a stride is below its row / frame").c_str());
    if (pixels && images->numFrames > 0 && !images->pixels) return fail(ctx, PS_ERR_BAD_ARG, (std::string(who) + ": null pixels").c_str());
    return PS_OK;
}

// The least non-negative double x, +inf included, with pred(x), for a predicate that is monotone in x and true at +inf:
// bisection over the bit patterns of the non-negative doubles, whose order is theirs.
template <class Pred> double least_double_where(Pred pred)
{
    const auto value = [](uint64_t bits) { double x; std::memcpy(&x, &bits, 8); return x; };
    uint64_t lo = 0, hi = 0x7FF0000000000000ull; // +inf
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (pred(value(mid))) hi = mid;
        else lo = mid + 1;
    }
    return value(lo);
}

} // namespace
