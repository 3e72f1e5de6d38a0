"""Device-resident frame sets and pair batches for ps_vo_pairs_device.

PyTorch is used here only as the HBM allocator / stream owner (torch.cuda on ROCm); all
compute happens in libputslam_hip.so behind the C ABI.
"""
import numpy as np
import torch

from . import api
from ._abi import (DMATCH_DTYPE, PS_VIEW_REQUIRE_VISIBLE, STATS_DTYPE, PsLoopBatch, PsLoopBatchF32, PsLoopResults, PsMapStore,
                   PsMapStoreF32, PsMapViewOut, PsMapViewOutF32, PsMapViewRequest, PsPoseSetOut, PsPoseSetOutF32, PsPoseSetRequest,
                   make_config, PsImageSet, klt_params, detect_params, orb_params, orb_detect_params, PsDepthSet, PsFrameRowsOut,
                   front_end_params, PsPointSets, PsTrackedCarry, PsTrackedRows, PsTrackVoIn, PsTrackVoOut, track_vo_params,
                   PsTrackCandidates, PsTrackCloseOut, track_close_params, PsUncertaintyOut, PsMeasurementEdgesOut, sensor_model,
                   PsPatchModel, PsPatchParams, patch_params, PATCH_GIVEN_MODEL)


_NUMPY_OF = {torch.int32: np.int32, torch.float64: np.float64}


def to_device_tensor(a, dtype, device, shape=None):
    """A contiguous tensor of `dtype` on `device`: a numpy array (or sequence) is converted, reshaped to `shape` if given, and
    uploaded; a device tensor is checked and used where it lies."""
    if isinstance(a, torch.Tensor):
        assert a.dtype == dtype and a.is_contiguous() and a.device == device
        return a
    a = np.ascontiguousarray(a, _NUMPY_OF[dtype])
    return torch.from_numpy(a if shape is None else a.reshape(shape)).to(device)


def _zeros(device, shape, dtype):
    return torch.zeros(shape, dtype=dtype, device=device)


def _expect(t, dtype, shape):
    """`t` is a contiguous tensor of this dtype and shape."""
    assert t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.is_contiguous(), (t.dtype, tuple(t.shape), dtype, tuple(shape))


def _block(t, device, shape, dtype):
    """The caller's block `t`, checked, or a new zeroed one of this shape."""
    t = _zeros(device, shape, dtype) if t is None else t
    _expect(t, dtype, shape)
    return t


def pack_frames(desc, pts, stride=None):
    """(F, cap, 32) u8 + (F, cap, 3) f32 -> (F, stride) u8: every frame one block [cap x 32 B descriptors][cap x 12 B points]
    padded to `stride` bytes (default: cap x 44 rounded up to 16 -- PS_FRAMES_PACKED / ps_vo_stream_packed_stride)."""
    F, cap = desc.shape[:2]
    stride = ((cap * 44 + 15) // 16) * 16 if stride is None else int(stride)
    out = np.zeros((F, stride), np.uint8)
    out[:, :cap * 32] = np.ascontiguousarray(desc, np.uint8).reshape(F, cap * 32)
    out[:, cap * 32:cap * 44] = np.ascontiguousarray(pts, np.float32).reshape(F, cap * 3).view(np.uint8)
    return out


def unpack_frames(blocks, cap):
    """pack_frames' inverse: (F, stride) u8 -> desc (F, cap, 32) u8, pts (F, cap, 3) f32."""
    desc = blocks[:, :cap * 32].reshape(-1, cap, 32)
    return desc, np.ascontiguousarray(blocks[:, cap * 32:cap * 44]).view(np.float32).reshape(-1, cap, 3)


class FrameSet:
    """desc + pts + nkpts (num_frames,) i32 of num_frames frames of capacity max_kpts in HBM.  stride None: dense, desc
    (F, cap, 32) u8 and pts (F, cap, 3) f32; else packed, blocks (F, stride) u8 as pack_frames lays them out (PsFrameSet strides).
    The subclasses fill it: FrameSetDevice / PackedFrameSetDevice upload, MapViewsDevice / PoseSetsDevice are written by the library."""

    stride = None

    def _zero_frames(self, n, packed_stride):
        """n zero-filled frames in the layout `packed_stride` asks for (None: dense)."""
        cap, dev = self.max_kpts, self.device
        self.stride = None if packed_stride is None else int(packed_stride)
        if self.stride is None:
            self.desc, self.pts = _zeros(dev, (n, cap, 32), torch.uint8), _zeros(dev, (n, cap, 3), torch.float32)
        else:
            self.blocks = _zeros(dev, (n, self.stride), torch.uint8)
        self.nkpts = _zeros(dev, (n,), torch.int32)

    def view(self):
        if self.stride is None:
            return api.DeviceFrames(self.desc.data_ptr(), self.pts.data_ptr(), self.nkpts.data_ptr(), self.num_frames,
                                    self.max_kpts)
        base = self.blocks.data_ptr()
        return api.DeviceFrames(base, base + self.max_kpts * 32, self.nkpts.data_ptr(), self.num_frames, self.max_kpts,
                                self.stride, self.stride)

    def frame_set(self):
        return self.view().struct()

    def download_frames(self):
        """(desc (F, cap, 32), pts (F, cap, 3)) on the host (numpy) whatever the layout."""
        if self.stride is None:
            return self.desc.cpu().numpy(), self.pts.cpu().numpy()
        return unpack_frames(self.blocks.cpu().numpy(), self.max_kpts)


class FrameSetDevice(FrameSet):
    """desc (F,cap,32) u8, pts (F,cap,3) f32, nkpts (F,) i32 resident in HBM."""

    def __init__(self, desc, pts, nkpts, device="cuda:0"):
        desc = np.ascontiguousarray(desc, np.uint8)
        pts = np.ascontiguousarray(pts, np.float32)
        nkpts = np.ascontiguousarray(nkpts, np.int32)
        assert desc.ndim == 3 and desc.shape[2] == 32 and pts.shape == desc.shape[:2] + (3,)
        self.device = torch.device(device)
        self.desc = torch.from_numpy(desc).to(self.device)
        self.pts = torch.from_numpy(pts).to(self.device)
        self.nkpts = torch.from_numpy(nkpts).to(self.device)
        self.num_frames, self.max_kpts = desc.shape[0], desc.shape[1]


class PackedFrameSetDevice(FrameSet):
    """The same frames as FrameSetDevice with every frame's descriptors and points in ONE block (PsFrameSet strides, ABI 2)."""

    def __init__(self, desc, pts, nkpts, device="cuda:0", stride=None):
        self.device = torch.device(device)
        packed = pack_frames(desc, pts, stride)
        self.num_frames, self.max_kpts = desc.shape[0], desc.shape[1]
        self.stride = packed.shape[1]
        self.blocks = torch.from_numpy(packed).to(self.device)
        self.nkpts = torch.from_numpy(np.ascontiguousarray(nkpts, np.int32)).to(self.device)


class FrameSetF32Device:
    """Float descriptors (F, cap, dim) f32, pts (F, cap, 3) f32 (or None: matching only) and nkpts (F,) i32 resident in HBM
    (PsFrameSetF32).  row_floats > dim: the rows lie row_floats floats apart and what lies between them is filled with `pad`
    (never read by the library)."""

    def __init__(self, desc, pts, nkpts, device="cuda:0", row_floats=None, pad=np.nan):
        desc = np.ascontiguousarray(desc, np.float32)
        assert desc.ndim == 3
        self.device = torch.device(device)
        self.num_frames, self.max_kpts, self.dim = desc.shape
        self.row_floats = self.dim if row_floats is None else int(row_floats)
        assert self.row_floats >= self.dim
        if self.row_floats != self.dim:
            wide = np.full((self.num_frames, self.max_kpts, self.row_floats), pad, np.float32)
            wide[:, :, :self.dim] = desc
            desc = wide
        self.desc = torch.from_numpy(desc).to(self.device)
        self.pts = None
        if pts is not None:
            pts = np.ascontiguousarray(pts, np.float32)
            assert pts.shape == (self.num_frames, self.max_kpts, 3)
            self.pts = torch.from_numpy(pts).to(self.device)
        self.nkpts = torch.from_numpy(np.ascontiguousarray(nkpts, np.int32)).to(self.device)

    def view(self):
        dense = self.row_floats == self.dim
        return api.DeviceFramesF32(self.desc.data_ptr(), 0 if self.pts is None else self.pts.data_ptr(), self.nkpts.data_ptr(),
                                   self.num_frames, self.max_kpts, self.dim, 0 if dense else self.row_floats * 4,
                                   0 if dense else self.max_kpts * self.row_floats * 4, 0)


class PairResultsDevice:
    """The per-pair output block in HBM (PsPairResults) for P pairs of `cap` rows: matches (P, cap, 16) u8, num_matches (P,)
    i32, mask (P, cap) u8, pose (P, 16) f32, stats (P, sizeof PsRansacStats) u8.  A subclass uploads and fills what else it
    needs first and calls this constructor last: every block is ready when it returns."""

    def __init__(self, P, cap, device):
        self.device = torch.device(device)
        self.P, self.cap = int(P), int(cap)
        P, cap = max(self.P, 1), self.cap
        self.matches = torch.zeros((P, cap, 16), dtype=torch.uint8, device=self.device)
        self.num_matches = torch.zeros(P, dtype=torch.int32, device=self.device)
        self.mask = torch.zeros((P, cap), dtype=torch.uint8, device=self.device)
        self.pose = torch.zeros((P, 16), dtype=torch.float32, device=self.device)
        self.stats = torch.zeros((P, STATS_DTYPE.itemsize), dtype=torch.uint8, device=self.device)
        # torch fills the blocks on its current stream; the library's chains run on streams of their own that are NOT ordered with
        # it (non-blocking streams): a fill still pending when a chain writes results would zero them afterwards (found by the queue
        # fuzz on batches of three pairs).  The blocks are ready when the constructor returns.
        torch.cuda.current_stream(self.device).synchronize()

    def view(self, lo=0):
        """DeviceResults of the rows from pair `lo` on."""
        m, n, k, p, s = self.matches, self.num_matches, self.mask, self.pose, self.stats
        if lo:
            m, n, k, p, s = m[lo:], n[lo:], k[lo:], p[lo:], s[lo:]
        return api.DeviceResults(m.data_ptr(), n.data_ptr(), k.data_ptr(), p.data_ptr(), s.data_ptr())

    def download(self):
        torch.cuda.synchronize(self.device)
        P = self.P
        return dict(matches=self.matches.cpu().numpy().view(DMATCH_DTYPE).reshape(max(P, 1), self.cap)[:P],
                    numMatches=self.num_matches.cpu().numpy()[:P],
                    inlierMask=self.mask.cpu().numpy()[:P],
                    pose=self.pose.cpu().numpy()[:P],
                    stats=self.stats.cpu().numpy().view(STATS_DTYPE).reshape(-1)[:P])


class PairBatchDevice(PairResultsDevice):
    """Pairs (P,2) i32 and the per-pair outputs, all in HBM."""

    def __init__(self, pairs, max_kpts, device="cuda:0"):
        pairs = np.ascontiguousarray(pairs, np.int32)
        self.pairs = torch.from_numpy(pairs).to(torch.device(device))
        super().__init__(pairs.shape[0], max_kpts, device)


_SIDE_STREAMS = {}


def _work_stream(device):
    """A non-default torch stream for the calling device.  The C ABI takes a hipStream_t and reads NULL as "the
    context's private stream", so torch's legacy default stream (handle 0) cannot be handed over: work submitted
    from the default stream runs on this side stream instead, forked from and joined back to the default stream."""
    key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(device=device)
    return _SIDE_STREAMS[key]


def _on_torch_stream(ctx, device, call, use_torch_stream=True):
    """call() -- one or more calls of `ctx` -- ordered after the work already queued on torch's current stream of `device`, which
    waits for what they queue (`_work_stream`: the default stream hands over through the side stream).  use_torch_stream=False:
    on whatever stream the context has."""
    if not use_torch_stream:
        call()
        return
    cur = torch.cuda.current_stream(device)
    if cur.cuda_stream != 0:
        ctx.set_stream(cur.cuda_stream)
        call()
        return
    st = _work_stream(device)
    st.wait_stream(cur)
    ctx.set_stream(st.cuda_stream)
    call()
    cur.wait_stream(st)


def run_pairs(ctx, params, cfg, K, frames: FrameSetDevice, batch: PairBatchDevice, use_torch_stream=True):
    """Asynchronous: match -> cross-check -> RANSAC -> refit for every pair of the batch, ordered after the work
    already queued on torch's current stream; the current stream waits for the results."""
    _on_torch_stream(ctx, frames.device,
                     lambda: ctx.vo_pairs_device(params, cfg, K, frames.view(), batch.pairs.data_ptr(), batch.P, batch.view()),
                     use_torch_stream)


def run_vo_pairs_l2(ctx, params, cfg, K, frames: FrameSetF32Device, batch: PairBatchDevice, use_torch_stream=True):
    """run_pairs for frames with float descriptors (ps_vo_pairs_l2_device)."""
    _on_torch_stream(ctx, frames.device,
                     lambda: ctx.vo_pairs_l2_device(params, cfg, K, frames.view(), batch.pairs.data_ptr(), batch.P, batch.view()),
                     use_torch_stream)


def run_match_l2(ctx, frames: FrameSetF32Device, batch: PairBatchDevice, use_torch_stream=True):
    """The matches alone (ps_match_l2_device) into batch.matches / batch.num_matches."""
    _on_torch_stream(ctx, frames.device,
                     lambda: ctx.match_l2_device(frames.view(), batch.pairs.data_ptr(), batch.P, batch.matches.data_ptr(),
                                                 batch.num_matches.data_ptr()),
                     use_torch_stream)


def run_pairs_split(ctxs, streams, params, estimator, num_hypotheses, seed, K, frames: FrameSetDevice,
                    batch: PairBatchDevice, bounds=None, join=True):
    """The same batch as `run_pairs`, submitted as len(ctxs) sub-batches on len(ctxs) HIP streams (`streams`: one
    non-default torch stream per context); every context owns its scratch arena, results land in disjoint slices of
    `batch`.  Pair p keeps its hypothesis stream (seed + p), so the outputs are bit-identical to the single call.
    join=True: every stream first waits for the current stream and the current stream waits for all of them at the
    end (the call is then ordered like `run_pairs`).  join=False: the sub-batch chains are only ordered within their
    own stream -- consecutive calls pipeline into each other and the caller synchronises before reading results."""
    S = len(ctxs)
    assert len(streams) >= S and all(st.cuda_stream != 0 for st in streams[:S])
    P = batch.P
    if bounds is None:
        # (two chains: 45 % / 55 % -- unequal sub-batches stay out of step, one chain's matrix-core Hamming sweep beside the
        # other's vector scoring sweep; equal ones march in lockstep and lose 2 - 3 %, profiles/r05k/chains_ab.txt)
        bounds = [0, int(P * 0.45), P] if (S == 2 and P >= 20) else [P * i // S for i in range(S + 1)]
    cur = torch.cuda.current_stream(frames.device)
    if join:
        for st in streams[:S]:
            st.wait_stream(cur)
    fv, keep = frames.view(), []
    for i in range(S):
        lo, hi = bounds[i], bounds[i + 1]
        if hi <= lo:
            continue
        ctxs[i].set_stream(streams[i].cuda_stream)
        ci, k = make_config(estimator, num_hypotheses, seed=seed + lo)
        keep.append(k)
        ctxs[i].vo_pairs_device(params, ci, K, fv, batch.pairs[lo:].data_ptr(), hi - lo, batch.view(lo))
    if join:
        for st in streams[:S]:
            cur.wait_stream(st)


def run_pairs_queue(queue, params, cfg, K, frames: FrameSetDevice, batch: PairBatchDevice):
    """The same batch as `run_pairs` through a PsBatchQueue (api.BatchQueue): the library hands the batches to its launch chains
    (two) in turn, whole; the chains are never joined, so consecutive batches run side by side -- give them output blocks of their
    own (two `PairBatchDevice`s used in turn).  Asynchronous; returns the batch's ticket -- `queue.wait(ticket)` (host),
    `queue.wait_on_stream(ticket, stream)` (a stream of the caller's) or `queue.synchronize()` before the results are read."""
    return queue.submit(params, cfg, K, frames.view(), batch.pairs.data_ptr(), batch.P, batch.view())


def dbscan_thin_device(ctx, xy, counts, octave=None, eps=10.0, min_pts=2, features_from_cluster=1):
    """DBScan keypoint thinning of a device-resident batch (ps_dbscan_thin_device): xy (F, cap, 2) float32, counts (F,) int32,
    octave (F, cap) int32 or None -- torch tensors on the context's device.  Returns (kept (F, cap) int32, nkept (F,) int32),
    device tensors written asynchronously on the context's stream: frame f keeps kept[f, :nkept[f]] (ascending)."""
    F, cap = xy.shape[0], xy.shape[1]
    _expect(xy, torch.float32, (F, cap, 2))
    _expect(counts, torch.int32, (F,))
    if octave is not None:
        _expect(octave, torch.int32, (F, cap))
    kept = torch.empty((F, cap), dtype=torch.int32, device=xy.device)
    nkept = torch.empty((F,), dtype=torch.int32, device=xy.device)
    args = (xy.data_ptr(), octave.data_ptr() if octave is not None else 0, counts.data_ptr(), F, cap, kept.data_ptr(),
            nkept.data_ptr(), eps, min_pts, features_from_cluster)
    _on_torch_stream(ctx, xy.device, lambda: ctx.dbscan_thin_device(*args))   # ordered like run_pairs
    return kept, nkept


def exclude_device(ctx, rule, cand3, cand2, cand_counts, exist3=None, exist2=None, exist_counts=None):
    """The exclusion filter `rule` (api.rule_*) over a device-resident batch (ps_exclude_device): cand3 (F, cap, 3) / cand2
    (F, cap, 2) float32, cand_counts (F,) int32; exist3 (F, ecap, 3) / exist2 (F, ecap, 2) / exist_counts (F,) or None -- torch
    tensors on the context's device; an array the rule does not read may be None.  Returns (kept (F, cap) int32, nkept (F,)
    int32), device tensors written asynchronously on the context's stream: frame f keeps kept[f, :nkept[f]] (ascending)."""
    lead = cand2 if cand2 is not None else cand3
    F, cap = lead.shape[0], lead.shape[1]
    for t, w in ((cand3, 3), (cand2, 2)):
        if t is not None:
            _expect(t, torch.float32, (F, cap, w))
    _expect(cand_counts, torch.int32, (F,))
    elead = exist2 if exist2 is not None else exist3
    ecap = 0 if elead is None else elead.shape[1]
    if ecap:
        for t, w in ((exist3, 3), (exist2, 2)):
            if t is not None:
                _expect(t, torch.float32, (F, ecap, w))
        _expect(exist_counts, torch.int32, (F,))
    kept = torch.empty((F, cap), dtype=torch.int32, device=lead.device)
    nkept = torch.empty((F,), dtype=torch.int32, device=lead.device)
    ptr = lambda t: t.data_ptr() if t is not None else 0   # noqa: E731
    args = (rule, ptr(cand3), ptr(cand2), cand_counts.data_ptr(), cap, ptr(exist3) if ecap else 0, ptr(exist2) if ecap else 0,
            exist_counts.data_ptr() if ecap else 0, ecap, F, kept.data_ptr(), nkept.data_ptr())
    _on_torch_stream(ctx, lead.device, lambda: ctx.exclude_device(*args))   # ordered like run_pairs
    return kept, nkept


def _image_set(images, rows, cols, channels):
    """PsImageSet of a uint8 device tensor (F, rows, cols[, channels]) whose rows and frames may lie any stride apart."""
    assert images.dtype == torch.uint8 and images.dim() in (3, 4) and tuple(images.shape[1:3]) == (rows, cols)
    cn = 1 if images.dim() == 3 else images.shape[3]
    assert cn == channels and (images.dim() == 3 and images.stride(2) == 1 or images.dim() == 4 and images.stride()[2:] == (cn, 1))
    return PsImageSet(images.data_ptr(), images.stride(1), images.stride(0) if images.shape[0] > 1 else 0, images.shape[0], rows, cols, cn)


class _Handle:
    """The owner of one handle of the library (`ctx`, `handle`): close() destroys it once, through the symbol the subclass's
    `_destroy` names, and so does the collector."""

    def close(self):
        if self.handle is not None:
            getattr(self.ctx._L, self._destroy)(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KltPyramids(_Handle):
    """A device-resident set of `slots` image pyramids with their derivatives (ps_klt_pyramids_create): the images of a sequence,
    built once, tracked pair by pair.  rows x cols x channels 8-bit images; win_size / max_levels as in _abi.klt_params."""

    _destroy = "ps_klt_pyramids_destroy"

    def __init__(self, ctx, rows, cols, channels, slots, win_size=7, max_levels=3):
        self.ctx, self.rows, self.cols, self.channels, self.slots = ctx, int(rows), int(cols), int(channels), int(slots)
        self.win_size, self.max_levels = int(win_size), int(max_levels)
        self.handle = ctx.klt_pyramids_create(rows, cols, channels, win_size, max_levels, slots)
        self.num_levels = int(ctx._L.ps_klt_pyramids_num_levels(self.handle))

    def build(self, images, first_slot=0, use_torch_stream=True):
        """Fills slots first_slot .. from `images`: a uint8 device tensor (F, rows, cols[, channels]) whose rows and frames may
        lie any stride apart (a view of a padded block); a row itself is dense.  Asynchronous, ordered like run_pairs."""
        s = _image_set(images, self.rows, self.cols, self.channels)
        _on_torch_stream(self.ctx, images.device, lambda: self.ctx.klt_pyramids_build_device(self.handle, s, first_slot),
                         use_torch_stream)

    def level(self, slot, level):
        """(image, derivative, (rows, cols)) of one stored level, border included, on the host (api.Context.debug_klt_level)."""
        return self.ctx.debug_klt_level(self.handle, slot, level, self.channels)


def track_klt_pairs(ctx, pyr: KltPyramids, pairs, prev_pts, counts, params=None, next_pts=None, status=None, err=None,
                    use_torch_stream=True):
    """cv::calcOpticalFlowPyrLK for P pairs of slots of `pyr` (ps_klt_track_device): pairs (P, 2) int32 (previous, next),
    prev_pts (P, cap, 2) float32, counts (P,) int32 -- torch tensors on the context's device.  next_pts: the initial flow under
    PS_KLT_USE_INITIAL_FLOW, written in place; status (P, cap) uint8 / err (P, cap) float32: blocks to write into (default: new
    ones).  Returns (next_pts, status, err), written asynchronously: nothing beyond a pair's count."""
    params = params or klt_params(pyr.win_size, pyr.max_levels)
    P, cap = prev_pts.shape[0], prev_pts.shape[1]
    dev = prev_pts.device
    _expect(prev_pts, torch.float32, (P, cap, 2))
    _expect(pairs, torch.int32, (P, 2))
    _expect(counts, torch.int32, (P,))
    next_pts = _block(next_pts, dev, (P, cap, 2), torch.float32)
    status = _block(status, dev, (P, cap), torch.uint8)
    err = _block(err, dev, (P, cap), torch.float32)
    args = (pyr.handle, params, pairs.data_ptr(), prev_pts.data_ptr(), counts.data_ptr(), P, cap, next_pts.data_ptr(),
            status.data_ptr(), err.data_ptr())
    _on_torch_stream(ctx, dev, lambda: ctx.klt_track_device(*args), use_torch_stream)
    return next_pts, status, err


def select_tracked(ctx, next_pts, status, err, counts, tracking_error_threshold, min_reproj_distance, use_torch_stream=True):
    """performTracking's selection for P pairs (ps_klt_select_device) on what track_klt_pairs returned.  Returns (matches (P, cap, 4)
    int32 words of PsDMatch, num_matches (P,) int32, kept_pts (P, cap, 2) float32, kept_idx (P, cap) int32), written
    asynchronously: pair p keeps its first num_matches[p] rows (-1: a count outside 0 .. cap)."""
    P, cap = status.shape
    dev = status.device
    _expect(next_pts, torch.float32, (P, cap, 2))
    _expect(status, torch.uint8, (P, cap))
    _expect(err, torch.float32, (P, cap))
    _expect(counts, torch.int32, (P,))
    matches = torch.empty((P, cap, 4), dtype=torch.int32, device=dev)
    num = torch.empty((P,), dtype=torch.int32, device=dev)
    kept_pts = torch.empty((P, cap, 2), dtype=torch.float32, device=dev)
    kept_idx = torch.empty((P, cap), dtype=torch.int32, device=dev)
    args = (next_pts.data_ptr(), status.data_ptr(), err.data_ptr(), counts.data_ptr(), P, cap, tracking_error_threshold,
            min_reproj_distance, matches.data_ptr(), num.data_ptr(), kept_pts.data_ptr(), kept_idx.data_ptr())
    _on_torch_stream(ctx, dev, lambda: ctx.klt_select_device(*args), use_torch_stream)
    return matches, num, kept_pts, kept_idx


class FastDetector(_Handle):
    """A device-resident FAST-9/16 detector for up to `max_frames` images of rows x cols x channels bytes a call
    (ps_fast_detector_create): the grey, score and corner maps of its last call stay readable through maps()."""

    _destroy = "ps_fast_detector_destroy"

    def __init__(self, ctx, rows, cols, channels, max_frames):
        self.ctx, self.rows, self.cols, self.channels, self.max_frames = ctx, int(rows), int(cols), int(channels), int(max_frames)
        self.handle = ctx.fast_detector_create(rows, cols, channels, max_frames)

    def maps(self, frame):
        """(grey, score, corner) of one frame of the last call, on the host (api.Context.debug_fast_maps)."""
        return self.ctx.debug_fast_maps(self.handle, frame, self.rows, self.cols)


def detect_features_batch(ctx, det: FastDetector, images, params=None, capacity=None, xy=None, response=None, counts=None,
                          use_torch_stream=True, passes=7):
    """MatcherOpenCV::detectFeatures (detector = "FAST") for every frame of `images` (ps_detect_features_device): a uint8 device
    tensor (F, rows, cols[, channels]) of the detector's shape, the tensor KltPyramids.build takes.  params: _abi.detect_params(...),
    default the shipped ones; capacity: rows per frame (default maximalTrackedFeatures).  xy (F, cap, 2) float32 / response (F, cap)
    float32 / counts (F,) int32: blocks to write into (default: new ones).  Returns (xy, response, counts), written asynchronously:
    nothing beyond a frame's count.  xy and counts drop into dbscan_thin_device, the rows it keeps into track_klt_pairs.
    passes: 7, or the mask of ps_debug_fast_passes (timing scripts)."""
    params = params or detect_params()
    s = _image_set(images, det.rows, det.cols, det.channels)
    F, dev = images.shape[0], images.device
    cap = int(params.maximalTrackedFeatures) if capacity is None else int(capacity)
    xy = _block(xy, dev, (F, cap, 2), torch.float32)
    response = _block(response, dev, (F, cap), torch.float32)
    counts = _block(counts, dev, (F,), torch.int32)
    args = (det.handle, s, params, cap, xy.data_ptr(), response.data_ptr(), counts.data_ptr(), passes)
    _on_torch_stream(ctx, dev, lambda: ctx.detect_features_device(*args), use_torch_stream)
    return xy, response, counts


class OrbDetector(_Handle):
    """A device-resident ORB detector for up to `max_frames` images of rows x cols x channels bytes a call (ps_orb_detector_create):
    one pyramid per (frame, ROI) of the grid of `params` (_abi.orb_detect_params(...), default the shipped ones), whose
    scaleFactor, nLevels, gridRows and gridCols are fixed here.  The planes and survivor lists of its last call stay readable
    through level()."""

    _destroy = "ps_orb_detector_destroy"

    def __init__(self, ctx, rows, cols, channels, max_frames, params=None):
        self.ctx, self.rows, self.cols, self.channels, self.max_frames = ctx, int(rows), int(cols), int(channels), int(max_frames)
        self.params = params or orb_detect_params()
        self.num_levels = int(self.params.nLevels)
        self.num_rois = int(self.params.gridRows) * int(self.params.gridCols)
        self.handle = ctx.orb_detector_create(rows, cols, channels, self.params, max_frames)

    def level_shape(self, level):
        """((rows, cols), scale float32) of one level of an ROI's pyramid (ps_orb_detector_level)."""
        return self.ctx.orb_detector_level(self.handle, level)

    def level(self, frame, roi, level):
        """The planes and lists of one level of ROI `roi` (loop order) of frame `frame` of the last call, on the host
        (api.Context.debug_orb_detect_level)."""
        return self.ctx.debug_orb_detect_level(self.handle, int(frame) * self.num_rois + int(roi), level)


def detect_features_orb_batch(ctx, det: OrbDetector, images, params=None, capacity=None, xy=None, response=None, angle=None, octave=None,
                              counts=None, use_torch_stream=True, passes=63):
    """MatcherOpenCV::detectFeatures (detector = "ORB") for every frame of `images` (ps_orb_detect_frames): a uint8 device tensor
    (F, rows, cols[, channels]) of the detector's shape.  params: _abi.orb_detect_params(...) with the detector's scaleFactor,
    nLevels and grid, default the detector's own; capacity: rows per frame (default maximalTrackedFeatures).  xy (F, cap, 2) float32 /
    response, angle (F, cap) float32 / octave (F, cap) int32 / counts (F,) int32: blocks to write into (default: new ones).  Returns
    (xy, response, angle, octave, counts), written asynchronously: nothing beyond a frame's count.  xy, octave and counts drop into
    dbscan_thin_device; xy, angle, octave and counts into describe_features_batch.  passes: 63, or the mask of
    ps_debug_orb_detect_passes (timing scripts)."""
    params = params or det.params
    s = _image_set(images, det.rows, det.cols, det.channels)
    F, dev = images.shape[0], images.device
    cap = int(params.maximalTrackedFeatures) if capacity is None else int(capacity)
    xy = _block(xy, dev, (F, cap, 2), torch.float32)
    response = _block(response, dev, (F, cap), torch.float32)
    angle = _block(angle, dev, (F, cap), torch.float32)
    octave = _block(octave, dev, (F, cap), torch.int32)
    counts = _block(counts, dev, (F,), torch.int32)
    args = (det.handle, s, params, cap, xy.data_ptr(), response.data_ptr(), angle.data_ptr(), octave.data_ptr(), counts.data_ptr(), passes)
    _on_torch_stream(ctx, dev, lambda: ctx.orb_detect_frames(*args), use_torch_stream)
    return xy, response, angle, octave, counts


class OrbPyramids(_Handle):
    """A device-resident set of `slots` ORB pyramids (ps_orb_pyramids_create): every level raw and blurred, with the sampling
    pattern -- (256, 4) int8 in -15 .. 15, default the library's.  params: _abi.orb_params(...), default cv::ORB::create()'s."""

    _destroy = "ps_orb_pyramids_destroy"

    def __init__(self, ctx, rows, cols, channels, slots, params=None, pattern=None):
        self.ctx, self.rows, self.cols, self.channels, self.slots = ctx, int(rows), int(cols), int(channels), int(slots)
        self.params = params or orb_params()
        self.num_levels = int(self.params.nLevels)
        self.handle = ctx.orb_pyramids_create(rows, cols, channels, self.params, pattern, slots)

    def build(self, images, first_slot=0, use_torch_stream=True, passes=7):
        """Fills slots first_slot .. from `images`: a uint8 device tensor (F, rows, cols[, channels]), the tensor KltPyramids.build
        and detect_features_batch take.  Asynchronous, ordered like run_pairs.  passes: 7, or the build mask of
        ps_debug_orb_passes (timing scripts)."""
        s = _image_set(images, self.rows, self.cols, self.channels)
        call = ((lambda: self.ctx.orb_pyramids_build_device(self.handle, s, first_slot)) if passes == 7 else
                (lambda: self.ctx.debug_orb_passes_build(self.handle, s, first_slot, passes)))
        _on_torch_stream(self.ctx, images.device, call, use_torch_stream)

    def level(self, level):
        """((rows, cols), scale float32) of one level (ps_orb_pyramids_level)."""
        return self.ctx.orb_pyramids_level(self.handle, level)

    def planes(self, slot, level):
        """(raw, blurred) of one level of one slot, on the host (api.Context.debug_orb_level)."""
        return self.ctx.debug_orb_level(self.handle, slot, level)


def describe_features_batch(ctx, pyr: OrbPyramids, slots, xy, angle, octave, counts, desc=None, kept_idx=None, num_kept=None,
                            use_torch_stream=True, passes=31):
    """MatcherOpenCV::describeFeatures (descriptor = "ORB") for F frames (ps_describe_features_device): slots (F,) int32 -- the
    slot of `pyr` each frame is described in --, xy (F, cap, 2) float32, angle (F, cap) float32 degrees, octave (F, cap) int32,
    counts (F,) int32: torch tensors on the context's device, the layout detect_features_batch returns.  desc (F, cap, 32) uint8 /
    kept_idx (F, cap) int32 / num_kept (F,) int32: blocks to write into (default: new ones).  Returns (desc, kept_idx, num_kept),
    written asynchronously: frame f's first num_kept[f] rows, grouped by octave, nothing beyond them (-1: a count outside
    0 .. cap).  desc drops into the binary frame sets."""
    F, cap = xy.shape[0], xy.shape[1]
    dev = xy.device
    _expect(xy, torch.float32, (F, cap, 2))
    _expect(angle, torch.float32, (F, cap))
    _expect(octave, torch.int32, (F, cap))
    for t in (slots, counts):
        _expect(t, torch.int32, (F,))
    desc = _block(desc, dev, (F, cap, 32), torch.uint8)
    kept_idx = _block(kept_idx, dev, (F, cap), torch.int32)
    num_kept = _block(num_kept, dev, (F,), torch.int32)
    args = (pyr.handle, slots.data_ptr(), xy.data_ptr(), angle.data_ptr(), octave.data_ptr(), counts.data_ptr(), F, cap, desc.data_ptr(),
            kept_idx.data_ptr(), num_kept.data_ptr(), passes)
    _on_torch_stream(ctx, dev, lambda: ctx.describe_features_device(*args), use_torch_stream)
    return desc, kept_idx, num_kept


def DepthSet(depth, rows, cols):
    """PsDepthSet of a uint16 (torch.int16 / torch.uint16) device tensor (F, rows, cols) whose rows and frames may lie any stride
    apart (a view of a padded block); a row itself is dense."""
    assert depth.element_size() == 2 and not depth.is_floating_point() and depth.dim() == 3 and tuple(depth.shape[1:]) == (rows, cols)
    assert depth.stride(2) == 1
    return PsDepthSet(depth.data_ptr(), depth.stride(1) * 2, depth.stride(0) * 2 if depth.shape[0] > 1 else 0, depth.shape[0], rows, cols)


def gather_keypoints(ctx, idx, nidx, xy, response=None, angle=None, octave=None, use_torch_stream=True):
    """Compacts F frames of key points by index lists (ps_gather_keypoints): idx (F, cap) int32 / nidx (F,) int32 -- what
    dbscan_thin_device returns --, xy (F, cap, 2) float32, response / angle (F, cap) float32, octave (F, cap) int32 or None.
    Returns (xy, response, angle, octave, counts) -- None where the input was None --, new device tensors written asynchronously:
    frame f's first counts[f] rows (-1: nidx[f] outside 0 .. cap), nothing beyond them.  They drop into describe_features_batch."""
    F, cap = xy.shape[0], xy.shape[1]
    dev = xy.device
    _expect(idx, torch.int32, (F, cap))
    _expect(nidx, torch.int32, (F,))
    _expect(xy, torch.float32, (F, cap, 2))
    for t, dt in ((response, torch.float32), (angle, torch.float32), (octave, torch.int32)):
        if t is not None:
            _expect(t, dt, (F, cap))
    like = lambda t: None if t is None else torch.zeros_like(t)   # noqa: E731
    ptr = lambda t: 0 if t is None else t.data_ptr()              # noqa: E731
    xy_o, resp_o, ang_o, oct_o = torch.zeros_like(xy), like(response), like(angle), like(octave)
    counts = _zeros(dev, (F,), torch.int32)
    args = (idx.data_ptr(), nidx.data_ptr(), F, cap, xy.data_ptr(), ptr(response), ptr(angle), ptr(octave), xy_o.data_ptr(), ptr(resp_o),
            ptr(ang_o), ptr(oct_o), counts.data_ptr())
    _on_torch_stream(ctx, dev, lambda: ctx.gather_keypoints(*args), use_torch_stream)
    return xy_o, resp_o, ang_o, oct_o, counts


_SIDE_ARRAYS = (("xy", torch.float32, (2,)), ("xy_undist", torch.float32, (2,)), ("angle", torch.float32, ()),
                ("response", torch.float32, ()), ("octave", torch.int32, ()), ("src_idx", torch.int32, ()), ("det_dist", torch.float64, ()))


class FrameRowsDevice(FrameSet):
    """What ps_assemble_frames / ps_front_end_frames write: a dense frame set -- desc (F, cap, 32) uint8 (assemble_frames leaves it
    zero: it writes no descriptors), pts (F, cap, 3) float32, nkpts (F,) int32: everything a FrameSetDevice is to run_pairs -- and
    the side arrays named in `side` (default all): xy, xy_undist (F, cap, 2) float32, angle, response (F, cap) float32, octave,
    src_idx (F, cap) int32, det_dist (F, cap) float64; the others are None."""

    def __init__(self, F, cap, device, side=None):
        self.device, self.num_frames, self.max_kpts = torch.device(device), int(F), int(cap)
        self._zero_frames(self.num_frames, None)
        names = [n for n, _, _ in _SIDE_ARRAYS] if side is None else list(side)
        for n, dt, tail in _SIDE_ARRAYS:
            setattr(self, n, _zeros(self.device, (self.num_frames, self.max_kpts) + tail, dt) if n in names else None)

    def out_struct(self, angle_in=None, response_in=None, octave_in=None):
        ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        return PsFrameRowsOut(ptr(self.pts), ptr(self.nkpts), ptr(self.xy), ptr(self.xy_undist), ptr(self.angle), ptr(self.response),
                              ptr(self.octave), ptr(self.src_idx), ptr(self.det_dist), ptr(angle_in), ptr(response_in), ptr(octave_in))

    def download(self):
        """dict of numpy arrays: desc, pts, nkpts and every side array that is there."""
        names = ["desc", "pts", "nkpts"] + [n for n, _, _ in _SIDE_ARRAYS if getattr(self, n) is not None]
        return {n: getattr(self, n).cpu().numpy() for n in names}


def assemble_frames(ctx, geometry, depth, xy, kept_idx, num_kept, angle=None, response=None, octave=None, first_depth_frame=0, side=None,
                    out=None, use_torch_stream=True):
    """Undistortion, back-projection and detection distance of the described key points in the described order
    (ps_assemble_frames): geometry _abi.frame_geometry(...); depth a uint16 device tensor (D, rows, cols), frame f reads depth frame
    first_depth_frame + f; xy (F, cap, 2) float32 and kept_idx (F, cap) int32 / num_kept (F,) int32 -- what describe_features_batch
    took and returned; angle / response / octave (F, cap): the key points' columns, needed where `side` names them.  side: the side
    arrays wanted (default: all whose input is there).  Returns a FrameRowsDevice, written asynchronously."""
    F, cap = xy.shape[0], xy.shape[1]
    dev = xy.device
    _expect(xy, torch.float32, (F, cap, 2))
    _expect(kept_idx, torch.int32, (F, cap))
    _expect(num_kept, torch.int32, (F,))
    if side is None:
        have = dict(angle=angle, response=response, octave=octave)
        side = [n for n, _, _ in _SIDE_ARRAYS if have.get(n, True) is not None]
    out = out or FrameRowsDevice(F, cap, dev, side)
    ds = DepthSet(depth, depth.shape[1], depth.shape[2])
    o = out.out_struct(angle, response, octave)
    _on_torch_stream(ctx, dev, lambda: ctx.assemble_frames(geometry, ds, first_depth_frame, xy.data_ptr(), kept_idx.data_ptr(),
                                                           num_kept.data_ptr(), F, cap, o), use_torch_stream)
    return out


class FrontEnd(_Handle):
    """The device-resident per-frame front end for up to `max_frames` images of rows x cols x channels bytes a call
    (ps_front_end_create): an ORB detector, an ORB pyramid set and every intermediate array.  params: _abi.front_end_params(...),
    default the shipped ones; pattern as OrbPyramids takes it."""

    _destroy = "ps_front_end_destroy"

    def __init__(self, ctx, rows, cols, channels, max_frames, params=None, pattern=None):
        self.ctx, self.rows, self.cols, self.channels, self.max_frames = ctx, int(rows), int(cols), int(channels), int(max_frames)
        self.params = params or front_end_params()
        self.handle = ctx.front_end_create(rows, cols, channels, self.params, pattern, max_frames)


def front_end_frames_batch(ctx, fe: FrontEnd, images, depth, geometry, capacity=None, side=None, out=None, use_torch_stream=True):
    """A batch of RGB-D images to a frame set (ps_front_end_frames): images a uint8 device tensor (F, rows, cols[, channels]) of the
    front end's shape, depth a uint16 device tensor (F, rows, cols), geometry _abi.frame_geometry(...); capacity: rows per frame
    (default max(1, maximalTrackedFeatures)).  Returns a FrameRowsDevice -- a frame set for run_pairs with the side arrays of
    `side` (default all) --, written asynchronously, ordered like run_pairs."""
    s = _image_set(images, fe.rows, fe.cols, fe.channels)
    ds = DepthSet(depth, fe.rows, fe.cols)
    F, dev = images.shape[0], images.device
    cap = max(1, int(fe.params.detect.maximalTrackedFeatures)) if capacity is None else int(capacity)
    out = out or FrameRowsDevice(F, cap, dev, side)
    o = out.out_struct()
    _on_torch_stream(ctx, dev, lambda: ctx.front_end_frames(fe.handle, s, ds, geometry, cap, out.desc.data_ptr(), o), use_torch_stream)
    return out


def run_image_sequence(ctx, fe: FrontEnd, images, depth, geometry, params, cfg, capacity=None, side=None, use_torch_stream=True):
    """Visual odometry over a sequence of RGB-D images with no host step: front_end_frames_batch, then run_pairs on the consecutive
    pairs (f, f + 1).  params / cfg: the RANSAC parameters and configuration of run_pairs; K is the geometry's.  Returns
    (frames: FrameRowsDevice, batch: PairBatchDevice), both written asynchronously."""
    frames = front_end_frames_batch(ctx, fe, images, depth, geometry, capacity, side, use_torch_stream=use_torch_stream)
    F = frames.num_frames
    pairs = np.stack([np.arange(0, max(F - 1, 0)), np.arange(1, max(F, 1))], axis=1).astype(np.int32)
    batch = PairBatchDevice(pairs, frames.max_kpts, frames.device)
    if batch.P:
        run_pairs(ctx, params, cfg, np.array(list(geometry.K), np.float32), frames, batch, use_torch_stream)
    return frames, batch


class PointSets:
    """S sets of 3-D points in HBM (PsPointSets): pts a float32 device tensor (S, cap, 3) whose sets may lie any stride apart (a
    view of a pitched block; a set itself is dense), counts (S,) int32."""

    def __init__(self, pts, counts):
        assert pts.dtype == torch.float32 and pts.dim() == 3 and pts.shape[2] == 3 and pts.stride()[1:] == (3, 1)
        _expect(counts, torch.int32, (pts.shape[0],))
        self.pts, self.counts, self.device = pts, counts, pts.device
        self.num_sets, self.capacity = int(pts.shape[0]), int(pts.shape[1])

    @classmethod
    def from_host(cls, sets, device, capacity=None, pitch_floats=None):
        """From a list of (n, 3) arrays: capacity rows a set (default the longest, at least 1), pitch_floats floats between sets
        (default dense); rows beyond a set's count and the pitch's padding are NaN."""
        cap = max([1] + [len(s) for s in sets]) if capacity is None else int(capacity)
        pitch = cap * 3 if pitch_floats is None else int(pitch_floats)
        block = np.full((max(len(sets), 1), pitch), np.nan, np.float32)
        for i, s in enumerate(sets):
            block[i, :len(s) * 3] = np.asarray(s, np.float32).reshape(-1)
        d = torch.from_numpy(block).to(torch.device(device))
        pts = d[:, :cap * 3].unflatten(1, (cap, 3))
        counts = torch.from_numpy(np.array([len(s) for s in sets] or [0], np.int32)).to(torch.device(device))
        return cls(pts, counts)

    def view(self):
        dense = self.num_sets == 1 or self.pts.stride(0) == self.capacity * 3
        return PsPointSets(self.pts.data_ptr(), self.counts.data_ptr(), self.num_sets, self.capacity, 0 if dense else self.pts.stride(0) * 4)


def ransac_match_lists(ctx, params, cfg, K, prev: PointSets, cur: PointSets, matches, num_matches, pairs=None, out=None,
                       use_torch_stream=True):
    """RANSAC / USAC over P caller-supplied device-resident match lists (ps_ransac_match_lists): matches (P, cap, 4) int32 words
    of PsDMatch -- what select_tracked returns --, num_matches (P,) int32, pairs (P, 2) int32 (previous set, current set) or None
    for (p, p).  Pair p draws from cfg.seed + p.  Returns a PairResultsDevice (mask, pose, stats; its matches / num_matches stay
    zero), written asynchronously, ordered like run_pairs."""
    P, cap = matches.shape[0], matches.shape[1]
    _expect(matches, torch.int32, (P, cap, 4))
    _expect(num_matches, torch.int32, (P,))
    if pairs is not None:
        _expect(pairs, torch.int32, (P, 2))
    out = out or PairResultsDevice(P, cap, matches.device)
    args = (params, cfg, K, prev.view(), cur.view(), None if pairs is None else pairs.data_ptr(), matches.data_ptr(), num_matches.data_ptr(),
            P, cap, out.view())
    _on_torch_stream(ctx, matches.device, lambda: ctx.ransac_match_lists_device(*args), use_torch_stream)
    return out


_TRACKED_ARRAYS = (("xy", torch.float32, (2,)), ("xy_undist", torch.float32, (2,)), ("pts", torch.float32, (3,)),
                   ("angle", torch.float32, ()), ("response", torch.float32, ()), ("octave", torch.int32, ()),
                   ("det_dist", torch.float64, ()))
_CARRIED = ("angle", "response", "octave", "det_dist")


class TrackedRows:
    """The rows a tracked frame leaves for P sequences (PsTrackedRows) -- and the previous rows the next frame's tracking starts
    from: xy, xy_undist (P, cap, 2), pts (P, cap, 3) float32, counts (P,) int32, and the carried columns named in `carried`
    (default all): angle, response (P, cap) float32, octave (P, cap) int32, det_dist (P, cap) float64; the others are None.
    track_vo_pairs takes one and returns one."""

    def __init__(self, P, cap, device, carried=_CARRIED):
        self.device, self.P, self.cap = torch.device(device), int(P), int(cap)
        for n, dt, tail in _TRACKED_ARRAYS:
            setattr(self, n, _zeros(self.device, (self.P, self.cap) + tail, dt) if n not in _CARRIED or n in carried else None)
        self.counts = _zeros(self.device, (self.P,), torch.int32)

    @property
    def carried(self):
        return tuple(n for n in _CARRIED if getattr(self, n) is not None)

    @classmethod
    def from_host(cls, device, xy, pts, counts, **columns):
        """Previous rows from numpy: xy (P, cap, 2), pts (P, cap, 3), counts (P,), and the carried columns by name."""
        xy = np.ascontiguousarray(xy, np.float32)
        r = cls(xy.shape[0], xy.shape[1], device, tuple(columns))
        r.xy.copy_(torch.from_numpy(xy))
        r.pts.copy_(torch.from_numpy(np.ascontiguousarray(pts, np.float32)))
        r.counts.copy_(torch.from_numpy(np.ascontiguousarray(counts, np.int32)))
        for n, a in columns.items():
            getattr(r, n).copy_(torch.from_numpy(np.ascontiguousarray(a)))
        return r

    def carry_struct(self):
        ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        return PsTrackedCarry(ptr(self.angle), ptr(self.response), ptr(self.octave), ptr(self.det_dist))

    def rows_struct(self):
        ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        return PsTrackedRows(ptr(self.xy), ptr(self.xy_undist), ptr(self.pts), ptr(self.counts), ptr(self.angle), ptr(self.response),
                             ptr(self.octave), ptr(self.det_dist))

    def download(self):
        names = ["counts"] + [n for n, _, _ in _TRACKED_ARRAYS if getattr(self, n) is not None]
        return {n: getattr(self, n).cpu().numpy() for n in names}


def assemble_tracked(ctx, geometry, depth, depth_frame, next_pts, kept_idx, num_kept, prev: TrackedRows = None, out: TrackedRows = None,
                     use_torch_stream=True):
    """The rows of the tracked points (ps_assemble_tracked): geometry _abi.frame_geometry(...); depth a uint16 device tensor (D, rows,
    cols), pair p reads depth frame depth_frame[p] ((P,) int32); next_pts (P, cap, 2) float32, kept_idx (P, cap) / num_kept (P,) int32
    -- what track_klt_pairs and select_tracked returned; prev: the previous rows whose carried columns go along by index (None:
    nothing is carried).  Returns a TrackedRows, written asynchronously."""
    P, cap = next_pts.shape[0], next_pts.shape[1]
    dev = next_pts.device
    _expect(next_pts, torch.float32, (P, cap, 2))
    _expect(kept_idx, torch.int32, (P, cap))
    _expect(num_kept, torch.int32, (P,))
    _expect(depth_frame, torch.int32, (P,))
    out = out or TrackedRows(P, cap, dev, prev.carried if prev is not None else ())
    ds = DepthSet(depth, depth.shape[1], depth.shape[2])
    carry = None if prev is None else prev.carry_struct()
    rows = out.rows_struct()
    _on_torch_stream(ctx, dev, lambda: ctx.assemble_tracked_device(geometry, ds, depth_frame.data_ptr(), next_pts.data_ptr(),
                                                                   kept_idx.data_ptr(), num_kept.data_ptr(), P, cap, carry, rows),
                     use_torch_stream)
    return out


class TrackVoDevice(PairResultsDevice):
    """Everything ps_track_vo_pairs writes for P pairs of `cap` rows: the tracker's next_pts (P, cap, 2) float32, status (P, cap)
    uint8, err (P, cap) float32; the selection's matches / num_matches (PairResultsDevice's) and kept_idx (P, cap) int32; the
    frame's rows (a TrackedRows); mask, pose, stats."""

    def __init__(self, P, cap, device, carried=_CARRIED):
        dev = torch.device(device)
        self.next_pts = _zeros(dev, (P, cap, 2), torch.float32)
        self.status = _zeros(dev, (P, cap), torch.uint8)
        self.err = _zeros(dev, (P, cap), torch.float32)
        self.kept_idx = _zeros(dev, (P, cap), torch.int32)
        self.rows = TrackedRows(P, cap, dev, carried)
        super().__init__(P, cap, dev)

    def out_struct(self):
        return PsTrackVoOut(self.next_pts.data_ptr(), self.status.data_ptr(), self.err.data_ptr(), self.matches.data_ptr(),
                            self.num_matches.data_ptr(), self.kept_idx.data_ptr(), self.rows.rows_struct(), self.mask.data_ptr(),
                            self.pose.data_ptr(), self.stats.data_ptr())

    def download(self):
        res = super().download()
        res.update(next_pts=self.next_pts.cpu().numpy(), status=self.status.cpu().numpy(), err=self.err.cpu().numpy(),
                   kept_idx=self.kept_idx.cpu().numpy(), rows=self.rows.download())
        return res


def track_vo_pairs(ctx, pyr: KltPyramids, depth, geometry, pairs, rows: TrackedRows, params, cfg, tp=None, klt=None, depth_frame=None,
                   out: TrackVoDevice = None, use_torch_stream=True):
    """The tracking VO step for P pairs of slots of `pyr` with no host step (ps_track_vo_pairs): track the previous rows' xy, select,
    assemble the tracked rows in the pair's depth frame (depth_frame (P,) int32; None: the pair's current slot) and run the estimator
    on (rows.pts, the new pts, the selection's matches).  pairs (P, 2) int32; rows: the previous frame's TrackedRows; params / cfg as
    for run_pairs (params.errorVersion is used as given); tp _abi.track_vo_params(...), klt _abi.klt_params(...).  Returns a
    TrackVoDevice, written asynchronously; its .rows are the `rows` of the next frame's call."""
    P, cap = rows.P, rows.cap
    _expect(pairs, torch.int32, (P, 2))
    if depth_frame is not None:
        _expect(depth_frame, torch.int32, (P,))
    tp = tp or track_vo_params()
    klt = klt or klt_params(pyr.win_size, pyr.max_levels)
    out = out or TrackVoDevice(P, cap, rows.device, rows.carried)
    ds = DepthSet(depth, depth.shape[1], depth.shape[2])
    vin = PsTrackVoIn(pairs.data_ptr(), None if depth_frame is None else depth_frame.data_ptr(), rows.xy.data_ptr(), rows.pts.data_ptr(),
                      rows.counts.data_ptr(), rows.carry_struct())
    o = out.out_struct()
    _on_torch_stream(ctx, rows.device, lambda: ctx.track_vo_pairs_device(pyr.handle, klt, tp, params, cfg, geometry, ds, vin, P, cap, o),
                     use_torch_stream)
    return out


def run_tracked_sequences(ctx, pyr: KltPyramids, depth, rows0: TrackedRows, frames, geometry, params, cfg, tp=None, klt=None,
                          minimal_tracked_features=150, use_torch_stream=True):
    """S tracked sequences in lockstep with no host step: frames (S, K + 1) slots of `pyr` (and depth frames of `depth`), pair s of
    step k = (frames[s][k], frames[s][k + 1]); rows0: the rows of every sequence's first frame.  Step k's rows are handed to step
    k + 1 where they lie; every step's blocks are allocated first, then the K calls are queued, and the counts are read back once at
    the end.  Returns (steps: K TrackVoDevice, refill: (S,) int64 -- the first step whose rows count fewer than
    minimal_tracked_features points (OpenCVParams.minimalTrackedFeatures: where a host's refill is due), K where none does).  The
    call does not refill: the steps behind a due refill continue from the thinned rows."""
    frames = np.ascontiguousarray(frames, np.int32)
    S, K = frames.shape[0], frames.shape[1] - 1
    assert S == rows0.P
    dev = rows0.device
    pairs = [torch.from_numpy(np.ascontiguousarray(frames[:, k:k + 2])).to(dev) for k in range(K)]
    steps = [TrackVoDevice(S, rows0.cap, dev, rows0.carried) for _ in range(K)]
    rows = rows0
    for k in range(K):
        track_vo_pairs(ctx, pyr, depth, geometry, pairs[k], rows, params, cfg, tp, klt, None, steps[k], use_torch_stream)
        rows = steps[k].rows
    refill = np.full(S, K, np.int64)
    if K:
        if not use_torch_stream:
            ctx.synchronize()
        counts = torch.stack([s.rows.counts for s in steps]).cpu().numpy()   # (K, S): the one read-back
        for s in range(S):
            due = np.nonzero(counts[:, s] < int(minimal_tracked_features))[0]
            refill[s] = due[0] if due.size else K
    return steps, refill


class TrackClose(_Handle):
    """The intermediates of ps_track_close_pairs for calls of up to max_pairs pairs x max_rows rows (ps_track_close_create): the
    merged rows, their levels and the description's keptIdx -- allocated once, so that a call neither allocates nor waits."""

    _destroy = "ps_track_close_destroy"

    def __init__(self, ctx, max_pairs, max_rows):
        self.ctx, self.max_pairs, self.max_rows = ctx, int(max_pairs), int(max_rows)
        self.handle = ctx.track_close_create(max_pairs, max_rows)


def track_candidates(ctx, fe: FrontEnd, images, depth, geometry, capacity=None, out=None, use_torch_stream=True):
    """The refill's sandbox for F frames (ps_track_candidates; matcher.cpp:218-246): detect, DBScan, undistort, back-project and the
    detection distances, nothing described.  Arguments as front_end_frames_batch takes them.  Returns a FrameRowsDevice with every
    side array (its desc stays zero; nkpts are the candidate counts), written asynchronously -- the `cand` of track_close_pairs."""
    s = _image_set(images, fe.rows, fe.cols, fe.channels)
    ds = DepthSet(depth, fe.rows, fe.cols)
    F, dev = images.shape[0], images.device
    cap = max(1, int(fe.params.detect.maximalTrackedFeatures)) if capacity is None else int(capacity)
    out = out or FrameRowsDevice(F, cap, dev)
    o = out.out_struct()
    _on_torch_stream(ctx, dev, lambda: ctx.track_candidates_device(fe.handle, s, ds, geometry, cap, o), use_torch_stream)
    return out


class ClosedRows(FrameSet):
    """What ps_track_close_pairs writes for P pairs of out_cap rows: desc (P, out_cap, 32) uint8, rows -- a TrackedRows with every
    column, the previous rows of the next track_vo_pairs --, src_idx (P, out_cap) int32 (the tracked row, or capacity + i for
    candidate i) and refill (P,) int32 (0 not due, 1 merged, 2 due without candidates).  desc, rows.pts and rows.counts are a dense
    frame set (pts / nkpts name them): a ClosedRows is to run_pairs what a FrameSetDevice is."""

    def __init__(self, P, out_cap, device):
        self.device, self.num_frames, self.max_kpts = torch.device(device), int(P), int(out_cap)
        self.P, self.cap = self.num_frames, self.max_kpts
        self.rows = TrackedRows(self.P, self.cap, self.device)
        self.desc = _zeros(self.device, (self.P, self.cap, 32), torch.uint8)
        self.pts, self.nkpts = self.rows.pts, self.rows.counts
        self.src_idx = _zeros(self.device, (self.P, self.cap), torch.int32)
        self.refill = _zeros(self.device, (self.P,), torch.int32)
        torch.cuda.current_stream(self.device).synchronize()   # (PairResultsDevice's reason: the blocks are ready when this returns)

    def out_struct(self):
        return PsTrackCloseOut(self.desc.data_ptr(), self.rows.rows_struct(), self.src_idx.data_ptr(), self.refill.data_ptr())

    def download(self):
        return dict(desc=self.desc.cpu().numpy(), src_idx=self.src_idx.cpu().numpy(), refill=self.refill.cpu().numpy(),
                    rows=self.rows.download())


def track_close_pairs(ctx, tc: TrackClose, pyr: OrbPyramids, slots, rows: TrackedRows, cand: FrameRowsDevice = None, cand_frame=None,
                      tp=None, out_cap=None, out: ClosedRows = None, use_torch_stream=True, passes=15):
    """matcher.cpp:213-381 for P pairs with no host step (ps_track_close_pairs): rows -- the TrackedRows a track_vo_pairs call left,
    every column --, cand -- what track_candidates returned, or None -- with cand_frame (P,) int32 (-1: none for that pair), pyr /
    slots (P,) int32: the built ORB pyramids and the slot of every pair's current image; tp _abi.track_close_params(...).  The refill
    is decided on the device (rows.counts[p] < minimalTrackedFeatures).  Returns a ClosedRows of out_cap rows (default rows.cap +
    cand's), written asynchronously; its .rows are the `rows` of the next track_vo_pairs.  passes: 15, or the mask of
    ps_debug_track_close_passes (timing scripts)."""
    P, cap = rows.P, rows.cap
    _expect(slots, torch.int32, (P,))
    tp = tp or track_close_params()
    cs = None
    if cand is not None:
        _expect(cand_frame, torch.int32, (P,))
        cs = PsTrackCandidates(cand.xy.data_ptr(), cand.xy_undist.data_ptr(), cand.pts.data_ptr(), cand.angle.data_ptr(),
                               cand.response.data_ptr(), cand.octave.data_ptr(), cand.det_dist.data_ptr(), cand.nkpts.data_ptr(),
                               cand.num_frames, cand.max_kpts)
    need = cap + (cand.max_kpts if cand is not None else 0)
    out_cap = (out.cap if out is not None else need) if out_cap is None else int(out_cap)
    out = out or ClosedRows(P, out_cap, rows.device)
    assert out.P == P and out.cap == out_cap
    o, r = out.out_struct(), rows.rows_struct()
    cf = None if cand is None else cand_frame.data_ptr()
    _on_torch_stream(ctx, rows.device, lambda: ctx.track_close_pairs_device(tc.handle, pyr.handle, slots.data_ptr(), tp, r, cs, cf, P, cap,
                                                                            out_cap, o, passes), use_torch_stream)
    return out


def run_tracked_vo(ctx, klt: KltPyramids, orb: OrbPyramids, fe: FrontEnd, tc: TrackClose, images, depth, rows0: TrackedRows, frames,
                   geometry, params, cfg, tp=None, klt_p=None, close_tp=None, cand_capacity=None, candidates="always",
                   use_torch_stream=True):
    """S tracked sequences in lockstep for K frames with the refill done on the device (matcher.cpp:147-381 per frame): frames
    (S, K + 1) name, for every sequence, the frames of `images` / `depth` -- device tensors (N, rows, cols[, channels]) uint8 and
    (N, rows, cols) uint16 -- which are also the slots of `klt` and `orb`, both built from `images` by the caller (one build
    serves every sequence and step).  rows0: the rows of every sequence's first frame, every column.  Per step: track_vo_pairs,
    the candidates, track_close_pairs; the closed rows are the next step's previous rows where they lie.  Two policies, both on
    the same calls: candidates="always" queues track_candidates for every sequence's current frame at every step and reads
    nothing back until the end (the device ignores candidates of a pair that is not due); candidates="due" reads the tracked
    counts back once a step and detects only for the sequences that are due.  A step's blocks hold cand_capacity rows more than
    the step before (ps_track_close_pairs' out-capacity rule), so a chain is as long as the handle `tc` has rows for.  Returns
    (steps: K TrackVoDevice -- poses, masks, statistics --, closed: K ClosedRows -- the frame sets --, counts (K, S), refill
    (K, S) int32 numpy: the closed rows' counts and ps_track_close_pairs' flags)."""
    assert candidates in ("always", "due")
    frames = np.ascontiguousarray(frames, np.int32)
    S, K = frames.shape[0], frames.shape[1] - 1
    assert S == rows0.P and rows0.carried == _CARRIED
    dev = rows0.device
    ccap = max(1, int(fe.params.detect.maximalTrackedFeatures)) if cand_capacity is None else int(cand_capacity)
    close_tp = close_tp or track_close_params()
    pairs = [torch.from_numpy(np.ascontiguousarray(frames[:, k:k + 2])).to(dev) for k in range(K)]
    slots = [torch.from_numpy(np.ascontiguousarray(frames[:, k + 1])).to(dev) for k in range(K)]
    steps = [TrackVoDevice(S, rows0.cap + k * ccap, dev) for k in range(K)]
    closed = [ClosedRows(S, rows0.cap + (k + 1) * ccap, dev) for k in range(K)]
    every = torch.arange(S, dtype=torch.int32, device=dev)
    rows = rows0
    for k in range(K):
        track_vo_pairs(ctx, klt, depth, geometry, pairs[k], rows, params, cfg, tp, klt_p, None, steps[k], use_torch_stream)
        cand, cand_frame = None, None
        if candidates == "always":
            cur = slots[k].long()
            cand, cand_frame = track_candidates(ctx, fe, images[cur], depth[cur], geometry, ccap, use_torch_stream=use_torch_stream), every
        else:
            if not use_torch_stream:
                ctx.synchronize()
            n = steps[k].rows.counts.cpu().numpy()      # (the step's one read-back)
            due = np.nonzero((n >= 0) & (n < int(close_tp.minimalTrackedFeatures)))[0]
            if due.size:
                cur = torch.from_numpy(frames[due, k + 1].astype(np.int64)).to(dev)
                cand = track_candidates(ctx, fe, images[cur], depth[cur], geometry, ccap, use_torch_stream=use_torch_stream)
                where = np.full(S, -1, np.int32)
                where[due] = np.arange(due.size, dtype=np.int32)
                cand_frame = torch.from_numpy(where).to(dev)
        if cand is None:    # nobody is due: the call still closes every sequence's rows
            track_close_pairs(ctx, tc, orb, slots[k], steps[k].rows, None, None, close_tp, out=closed[k], use_torch_stream=use_torch_stream)
        else:
            track_close_pairs(ctx, tc, orb, slots[k], steps[k].rows, cand, cand_frame, close_tp, out=closed[k],
                              use_torch_stream=use_torch_stream)
        rows = closed[k].rows
    if K and not use_torch_stream:
        ctx.synchronize()
    counts = torch.stack([c.rows.counts for c in closed]).cpu().numpy() if K else np.zeros((0, S), np.int32)
    refill = torch.stack([c.refill for c in closed]).cpu().numpy() if K else np.zeros((0, S), np.int32)
    return steps, closed, counts, refill


class MapBatchDevice(PairResultsDevice):
    """A map-matching batch in HBM (PsMapBatch): the map views and frames (FrameSetDevice / PackedFrameSetDevice), their levels
    (views x maxKpts / frames x maxKpts int32), pairs (P, 2) of (map view, frame), the sphere radius and accept ratio -- scalars, or
    sequences of P for per-pair values -- and the output block with `max_matches` rows per pair."""

    _batch_view_type = api.DeviceMapBatch   # (MapBatchF32Device: the float sets' struct)

    def __init__(self, maps, map_level, frames, cur_level, pairs, max_matches, radius=0.12, ratio=0.55, device=None):
        self.device = torch.device(device) if device is not None else maps.device
        self.maps, self.frames = maps, frames
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        self.P = pairs.shape[0]
        self.map_level = self._levels(map_level, maps)
        self.cur_level = self._levels(cur_level, frames)
        self.pairs = torch.from_numpy(pairs).to(self.device)
        self.radius_bound = self.accept_ratio = 0.0
        self.radius_per = self.ratio_per = None
        if np.ndim(radius) == 0:
            self.radius_bound = api.map_sphere_bound(radius)
        else:
            assert len(radius) == self.P
            self.radius_per = torch.from_numpy(np.array([api.map_sphere_bound(r) for r in radius], np.float32)).to(self.device)
        if np.ndim(ratio) == 0:
            self.accept_ratio = float(ratio)
        else:
            assert len(ratio) == self.P
            self.ratio_per = torch.from_numpy(np.array(ratio, np.float64)).to(self.device)
        super().__init__(self.P, max_matches, self.device)

    def _levels(self, level, fs):
        """Levels of a frame set: a numpy array is uploaded; a device tensor (build_map_views' / frame_levels_device's
        output) is used where it lies."""
        level = to_device_tensor(level, torch.int32, self.device)
        assert tuple(level.shape) == (fs.num_frames, fs.max_kpts)
        return level

    def batch_view(self, lo=0, hi=None):
        """PsMapBatch of pairs [lo, hi)."""
        hi = self.P if hi is None else hi
        return self._batch_view_type(self.maps.view(), self.map_level.data_ptr(), self.frames.view(), self.cur_level.data_ptr(),
                                  self.pairs[lo:].data_ptr() if lo < self.P else self.pairs.data_ptr(), hi - lo, self.cap,
                                  self.radius_bound, self.accept_ratio,
                                  self.radius_per[lo:].data_ptr() if self.radius_per is not None else None,
                                  self.ratio_per[lo:].data_ptr() if self.ratio_per is not None else None)


def run_map_pairs(ctx, params, cfg, K, batch: MapBatchDevice, use_torch_stream=True):
    """Asynchronous: guided map matching -> RANSAC -> refit for every pair of the batch (ps_map_pairs_device), ordered like
    `run_pairs`: after the work already queued on torch's current stream, which waits for the results."""
    _on_torch_stream(ctx, batch.device, lambda: ctx.map_pairs_device(params, cfg, K, batch.batch_view(), batch.view()),
                     use_torch_stream)


def run_match_xyz(ctx, batch: MapBatchDevice, use_torch_stream=True):
    """Asynchronous: the guided matching alone (ps_match_xyz_device) into the batch's matches / num_matches."""
    _on_torch_stream(ctx, batch.device,
                     lambda: ctx.match_xyz_device(batch.batch_view(), batch.matches.data_ptr(), batch.num_matches.data_ptr()),
                     use_torch_stream)


# ---- measurement uncertainty (ps_uncertainty.h) ----
_EDGE_ARRAYS = (("map_row", torch.int32, ()), ("cur_row", torch.int32, ()), ("uv", torch.float32, (2,)), ("position", torch.float64, (3,)),
                ("normal", torch.float64, (3,)), ("gradient", torch.float64, (3,)), ("info", torch.float64, (9,)))


class MeasurementEdges:
    """What ps_feature_uncertainty / ps_measurement_edges write for S row sets of `cap` rows: count (S,) int32 and the members
    named in `want` -- map_row, cur_row (S, cap) int32, uv (S, cap, 2) float32, position, normal, gradient (S, cap, 3) float64,
    info (S, cap, 9) float64, row-major --; the others are None.  The Edge3D(position, info, poseId, featureId) data of a batch.
    image_frame: the (frames,) int32 device tensor the call that wrote it read, kept alive here."""

    image_frame = None

    def __init__(self, S, cap, device, want=None, count=None):
        self.device, self.S, self.cap = torch.device(device), int(S), int(cap)
        names = [n for n, _, _ in _EDGE_ARRAYS] if want is None else list(want)
        self.count = _zeros(self.device, (max(self.S, 1),), torch.int32) if count is None else count
        for n, dt, tail in _EDGE_ARRAYS:
            setattr(self, n, _zeros(self.device, (max(self.S, 1), self.cap) + tail, dt) if n in names else None)

    def rows_struct(self):
        ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        return PsUncertaintyOut(ptr(self.normal), ptr(self.gradient), ptr(self.info))

    def edges_struct(self):
        ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        return PsMeasurementEdgesOut(ptr(self.count), ptr(self.map_row), ptr(self.cur_row), ptr(self.uv), ptr(self.position), ptr(self.normal),
                                     ptr(self.gradient), ptr(self.info))

    def download(self):
        """dict of numpy arrays: count and every member that is there."""
        names = ["count"] + [n for n, _, _ in _EDGE_ARRAYS if getattr(self, n) is not None]
        return {n: getattr(self, n).cpu().numpy()[:self.S] for n in names}


def _uncertainty_sets(images, depth, image_frame, frames, device):
    ds = DepthSet(depth, depth.shape[1], depth.shape[2])
    s = None if images is None else _image_set(images, depth.shape[1], depth.shape[2], 3)
    if not isinstance(image_frame, torch.Tensor):
        # uploaded on torch's current stream and waited for: a call made with use_torch_stream=False is ordered with nothing of torch's
        image_frame = to_device_tensor(np.arange(frames, dtype=np.int32) if image_frame is None else image_frame, torch.int32, device)
        torch.cuda.current_stream(device).synchronize()
    _expect(image_frame, torch.int32, (frames,))
    return s, ds, image_frame


def feature_uncertainty(ctx, rows, geometry, depth, images=None, sensor=None, model=-1, image_frame=None, want=("normal", "gradient", "info"),
                        out=None, use_torch_stream=True):
    """Normals, colour-gradient directions and information matrices of the rows of a FrameRowsDevice -- FrontEnd rows, or the
    survivors of exclude_device after gather_keypoints: anything with xy_undist (F, cap, 2), pts (F, cap, 3) and nkpts (F,) --
    with no host step (ps_feature_uncertainty; the addFeatures side, PUTSLAM.cpp:871-884).  depth a uint16 device tensor (D,
    rows, cols), images a uint8 device tensor (D, rows, cols, 3) or None where neither the gradient nor model 2 is wanted;
    image_frame (F,) int32: the frame of both that row set f belongs to (default f).  sensor: _abi.sensor_model(...).  Returns a
    MeasurementEdges with the members of `want`, written asynchronously, ordered like run_pairs."""
    F, cap, dev = rows.num_frames, rows.max_kpts, rows.device
    want = [w for w in want if not (w == "gradient" and images is None)]
    out = out or MeasurementEdges(F, cap, dev, want, count=rows.nkpts)
    s, ds, image_frame = _uncertainty_sets(images, depth, image_frame, F, dev)
    sensor = sensor or sensor_model()
    out.image_frame = image_frame      # (held: the queued kernel reads it)
    o = out.rows_struct()
    _on_torch_stream(ctx, dev, lambda: ctx.feature_uncertainty_device(geometry, sensor, model, s, ds, image_frame.data_ptr(),
                                                                       rows.xy_undist.data_ptr(), rows.pts.data_ptr(), rows.nkpts.data_ptr(),
                                                                       F, cap, o), use_torch_stream)
    return out


def measurement_edges(ctx, batch, xy_undist, geometry, depth, images=None, sensor=None, model=-1, image_frame=None, want=None, out=None,
                      use_torch_stream=True):
    """The measurements of a map batch as Edge3D data (ps_measurement_edges; the addMeasurements side, matcher.cpp:769-794 and
    featuresMap.cpp:255-282): batch a MapBatchDevice that run_map_pairs has filled (or is queued to fill: the call is ordered
    behind it), xy_undist (frames, maxKpts, 2) float32 -- the xy_undist of the FrameRowsDevice the batch's frames are.  Pair p's
    final inliers, in match-list order, fill the first count[p] rows.  Other arguments as feature_uncertainty.  Returns a
    MeasurementEdges of batch.P sets of batch.cap rows."""
    dev, frames = batch.device, batch.frames.num_frames
    _expect(xy_undist, torch.float32, (frames, batch.frames.max_kpts, 2))
    if want is None:
        want = [n for n, _, _ in _EDGE_ARRAYS if not (n == "gradient" and images is None)]
    out = out or MeasurementEdges(batch.P, batch.cap, dev, want)
    s, ds, image_frame = _uncertainty_sets(images, depth, image_frame, frames, dev)
    sensor = sensor or sensor_model()
    out.image_frame = image_frame      # (held: the queued kernel reads it)
    o = out.edges_struct()
    _on_torch_stream(ctx, dev, lambda: ctx.measurement_edges_device(geometry, sensor, model, s, ds, image_frame.data_ptr(), batch.batch_view(),
                                                                     batch.view(), xy_undist.data_ptr(), o), use_torch_stream)
    return out


class PatchModels:
    """The model arrays of P x cap points (PsPatchModel): patch (P, cap, E) float64, gx / gy (P, cap, E) float32, inv (P, cap, 9)
    float32, on `device`; `want` names the arrays to keep (the others are NULL: not written)."""

    def __init__(self, P, cap, patch_size, device, want=("patch", "gx", "gy", "inv")):
        E = int(patch_size) ** 2
        self.P, self.cap, self.E, self.device = P, cap, E, device
        self.patch = _zeros(device, (P, cap, E), torch.float64) if "patch" in want else None
        self.gx = _zeros(device, (P, cap, E), torch.float32) if "gx" in want else None
        self.gy = _zeros(device, (P, cap, E), torch.float32) if "gy" in want else None
        self.inv = _zeros(device, (P, cap, 9), torch.float32) if "inv" in want else None

    def struct(self):
        return PsPatchModel(*[t.data_ptr() if t is not None else None for t in (self.patch, self.gx, self.gy, self.inv)])


def _patch_images(images):
    assert images.dtype == torch.uint8 and images.dim() in (3, 4)
    return _image_set(images, images.shape[1], images.shape[2], 1 if images.dim() == 3 else images.shape[3])


def patch_models(ctx, images, slots, pts, counts, params=None, model: PatchModels = None, status=None, use_torch_stream=True):
    """computePatch + computeGradient for P sets of points (ps_patch_models): images a uint8 device tensor (F, rows, cols[, 3]) whose
    rows and frames may lie any stride apart, slots (P,) int32 the frame of each set, pts (P, cap, 2) float64, counts (P,) int32.
    Returns (model, status (P, cap) uint8), written asynchronously: nothing beyond a set's count."""
    params = params or patch_params()
    P, cap = pts.shape[0], pts.shape[1]
    dev = pts.device
    _expect(pts, torch.float64, (P, cap, 2))
    _expect(slots, torch.int32, (P,))
    _expect(counts, torch.int32, (P,))
    model = model or PatchModels(P, cap, params.patchSize, dev)
    status = _block(status, dev, (P, cap), torch.uint8)
    s = _patch_images(images)
    args = (s, slots.data_ptr(), pts.data_ptr(), counts.data_ptr(), P, cap, params, model.struct(), status.data_ptr())
    _on_torch_stream(ctx, dev, lambda: ctx.patch_models(*args), use_torch_stream)
    return model, status


def align_patches(ctx, images, pairs, old_pts, new_pts, counts, params=None, model: PatchModels = None, given=False, status=None,
                  iterations=None, use_torch_stream=True):
    """optimizeLocation for P pairs of frames (ps_patch_align): pairs (P, 2) int32 (old, new), old_pts / new_pts (P, cap, 2)
    float64 -- new_pts the starting guesses, refined IN PLACE --, counts (P,) int32.  model: where the fused call writes the model
    (None: nowhere); given=True: the model is read from it instead (PS_PATCH_GIVEN_MODEL; old_pts may be None).  Returns (new_pts,
    status (P, cap) uint8, iterations (P, cap) int32), written asynchronously: nothing beyond a pair's count."""
    params = params or patch_params()
    P, cap = new_pts.shape[0], new_pts.shape[1]
    dev = new_pts.device
    _expect(new_pts, torch.float64, (P, cap, 2))
    if old_pts is not None:
        _expect(old_pts, torch.float64, (P, cap, 2))
    _expect(pairs, torch.int32, (P, 2))
    _expect(counts, torch.int32, (P,))
    if given:
        assert model is not None
        params = PsPatchParams(params.minSqrtIncrement, params.patchSize, params.maxIter, params.flags | PATCH_GIVEN_MODEL, 0)
    status = _block(status, dev, (P, cap), torch.uint8)
    iterations = _block(iterations, dev, (P, cap), torch.int32)
    s = _patch_images(images)
    args = (s, pairs.data_ptr(), old_pts.data_ptr() if old_pts is not None else None, new_pts.data_ptr(), counts.data_ptr(), P, cap, params,
            model.struct() if model is not None else None, status.data_ptr(), iterations.data_ptr())
    _on_torch_stream(ctx, dev, lambda: ctx.patch_align(*args), use_torch_stream)
    return new_pts, status, iterations


class MapBatchF32Device(MapBatchDevice):
    """MapBatchDevice for float descriptors (PsMapBatchF32): maps / frames are FrameSetF32Device of one dim, with points."""

    def __init__(self, maps, map_level, frames, cur_level, pairs, max_matches, radius=0.12, ratio=0.55, device=None):
        assert maps.pts is not None and frames.pts is not None
        super().__init__(maps, map_level, frames, cur_level, pairs, max_matches, radius, ratio, device)

    _batch_view_type = api.DeviceMapBatchF32


def run_map_pairs_l2(ctx, params, cfg, K, batch: MapBatchF32Device, use_torch_stream=True):
    """run_map_pairs for float descriptors (ps_map_pairs_l2_device)."""
    _on_torch_stream(ctx, batch.device, lambda: ctx.map_pairs_l2_device(params, cfg, K, batch.batch_view(), batch.view()),
                     use_torch_stream)


def run_match_xyz_l2(ctx, batch: MapBatchF32Device, use_torch_stream=True):
    """run_match_xyz for float descriptors (ps_match_xyz_l2_device)."""
    _on_torch_stream(ctx, batch.device,
                     lambda: ctx.match_xyz_l2_device(batch.batch_view(), batch.matches.data_ptr(), batch.num_matches.data_ptr()),
                     use_torch_stream)


class MapStoreDevice:
    """The front-end feature map resident in HBM (PsMapStore), uploaded once and replaced whole: pos (F, 3) float64 global
    positions; obs_start (F + 1,) int32 -- feature f's observations are rows obs_start[f] .. obs_start[f + 1] of the observation
    arrays, ascending pose id; obs_pose (O,) int32, obs_desc (O, 32) uint8, obs_octave (O,) int32, obs_det_dist (O,) float64."""

    def __init__(self, pos, obs_start, obs_pose, obs_desc, obs_octave, obs_det_dist, num_poses, device="cuda:0"):
        self.device = torch.device(device)
        pos = np.ascontiguousarray(pos, np.float64).reshape(-1, 3)
        obs_start = np.ascontiguousarray(obs_start, np.int32)
        obs_pose = np.ascontiguousarray(obs_pose, np.int32)
        obs_desc = np.ascontiguousarray(obs_desc, np.uint8).reshape(-1, 32)
        obs_octave = np.ascontiguousarray(obs_octave, np.int32)
        obs_det_dist = np.ascontiguousarray(obs_det_dist, np.float64)
        self.num_features, self.num_obs, self.num_poses = pos.shape[0], obs_pose.shape[0], int(num_poses)
        assert obs_start.shape == (self.num_features + 1,)
        assert obs_desc.shape[0] == obs_octave.shape[0] == obs_det_dist.shape[0] == self.num_obs
        up = lambda a: torch.from_numpy(a).to(self.device)   # noqa: E731
        self.pos, self.obs_start, self.obs_pose = up(pos), up(obs_start), up(obs_pose)
        self.obs_desc, self.obs_octave, self.obs_det_dist = up(obs_desc), up(obs_octave), up(obs_det_dist)
        torch.cuda.current_stream(self.device).synchronize()   # (resident before a context's own stream reads it)

    def view(self):
        return PsMapStore(self.pos.data_ptr(), self.obs_start.data_ptr(), self.obs_pose.data_ptr(), self.obs_desc.data_ptr(),
                          self.obs_octave.data_ptr(), self.obs_det_dist.data_ptr(), self.num_features, self.num_obs,
                          self.num_poses, 0)


class MapViewsDevice(FrameSet):
    """What ps_map_views_device wrote: a frame set (desc / pts / nkpts; usable as MapBatchDevice.maps), map_level (V, cap) int32
    for MapBatchDevice's map_level, view_count (V,) and the side arrays feat_idx / obs_idx (V, cap) int32, pos_cam (V, cap, 3),
    uv (V, cap, 2), angle (V, cap) float64 -- device tensors.  packed_stride: bytes per view of ONE block
    [cap x 32 B descriptors][cap x 12 B points] (PsFrameSet strides) instead of two dense arrays."""

    def __init__(self, V, max_kpts, device, packed_stride=None):
        self.device = torch.device(device)
        self.num_frames, self.max_kpts = int(V), int(max_kpts)
        n, cap = max(self.num_frames, 1), self.max_kpts
        new = lambda shape, dt: _zeros(self.device, shape, dt)   # noqa: E731
        self._zero_frames(n, packed_stride)
        self.view_count = new((n,), torch.int32)
        self.map_level, self.feat_idx, self.obs_idx = (new((n, cap), torch.int32) for _ in range(3))
        self.pos_cam, self.uv, self.angle = new((n, cap, 3), torch.float64), new((n, cap, 2), torch.float64), new((n, cap), torch.float64)
        torch.cuda.current_stream(self.device).synchronize()   # (the fills are done before a context's stream writes)

    def out_struct(self):
        return PsMapViewOut(self.frame_set(), self.map_level.data_ptr(), self.view_count.data_ptr(), self.feat_idx.data_ptr(),
                            self.obs_idx.data_ptr(), self.pos_cam.data_ptr(), self.uv.data_ptr(), self.angle.data_ptr())

    def download(self):
        """Everything on the host (numpy); desc (V, cap, 32) and pts (V, cap, 3) whatever the layout."""
        torch.cuda.synchronize(self.device)
        V = self.num_frames
        desc, pts = self.download_frames()
        g = lambda t: t.cpu().numpy()[:V]   # noqa: E731
        return dict(desc=desc[:V], pts=pts[:V], nkpts=g(self.nkpts), viewCount=g(self.view_count), mapLevel=g(self.map_level),
                    featIdx=g(self.feat_idx), obsIdx=g(self.obs_idx), posCam=g(self.pos_cam), uv=g(self.uv), angle=g(self.angle))


def _map_view_request(store, cam_inv, pose_angle, max_angle, K, image_size, cand, cand_counts, require_visible):
    """(PsMapViewRequest, the device tensors it points to, V) for a store (MapStoreDevice / MapStoreF32Device)."""
    dev = store.device
    if not isinstance(cam_inv, torch.Tensor):
        cam_inv = np.ascontiguousarray(np.asarray(cam_inv, np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)).reshape(-1, 16)
    cam_inv = to_device_tensor(cam_inv, torch.float64, dev)
    V = int(cam_inv.shape[0])
    pose_angle = to_device_tensor(pose_angle, torch.float64, dev, (V, store.num_poses))
    assert tuple(pose_angle.shape) == (V, store.num_poses)
    req = PsMapViewRequest()
    req.camInv, req.poseAngle = cam_inv.data_ptr(), pose_angle.data_ptr()
    keep = [cam_inv, pose_angle]
    if cand is not None:
        cand, cand_counts = to_device_tensor(cand, torch.int32, dev), to_device_tensor(cand_counts, torch.int32, dev)
        assert cand.dim() == 2 and cand.shape[0] == V and tuple(cand_counts.shape) == (V,)
        # (a list of capacity 0 is still a list -- every view empty --, not "every feature": an empty tensor has no address)
        buf = cand if cand.numel() else torch.zeros(1, dtype=torch.int32, device=dev)
        req.cand, req.candCounts, req.candCapacity = buf.data_ptr(), cand_counts.data_ptr(), int(cand.shape[1])
        keep += [buf, cand_counts]
    req.maxAngle = float(max_angle)
    req.fx, req.fy, req.cx, req.cy = (float(x) for x in K)
    req.imageW, req.imageH = float(image_size[0]), float(image_size[1])
    req.V, req.flags = V, PS_VIEW_REQUIRE_VISIBLE if require_visible else 0
    return req, keep, V


def build_map_views(ctx, store: MapStoreDevice, cam_inv, pose_angle, max_angle, K, image_size, max_kpts, cand=None,
                    cand_counts=None, require_visible=False, out=None, packed_stride=None, use_torch_stream=True):
    """ps_map_views_device: V map views from the resident store, asynchronous, ordered like `run_map_pairs`.
    cam_inv (V, 4, 4): inverse camera poses (numpy, or a device tensor (V, 16) float64 column-major); pose_angle (V, num_poses):
    api.view_angles of each view's pose (numpy or device tensor); K = (fx, fy, cx, cy); image_size = (width, height);
    cand (V, cap) int32 + cand_counts (V,) (numpy or device tensors), or None = every feature of the store in index order.
    Returns a MapViewsDevice (`out`, if given, is written again: a retry with the reported capacity allocates a new one)."""
    dev = store.device
    req, keep, V = _map_view_request(store, cam_inv, pose_angle, max_angle, K, image_size, cand, cand_counts, require_visible)
    if out is None:
        out = MapViewsDevice(V, max_kpts, dev, packed_stride)
    assert out.num_frames >= V and out.max_kpts == int(max_kpts)
    torch.cuda.current_stream(dev).synchronize()   # (uploads above are complete before the context's stream reads them)
    out.inputs = keep                              # the request's device arrays live as long as the result
    st, os_ = store.view(), out.out_struct()
    _on_torch_stream(ctx, dev, lambda: ctx.map_views_device(st, req, os_), use_torch_stream)
    return out


def frame_levels_device(ctx, frames, octave, det_dist, use_torch_stream=True):
    """ps_frame_levels_device: predicted levels (F, cap) int32 of the keypoints of a device-resident frame set, for
    MapBatchDevice's cur_level.  octave (F, cap) int32 / det_dist (F, cap) float64: numpy or device tensors.  An octave outside
    the level table gives -1."""
    dev = frames.device
    octave, det_dist = to_device_tensor(octave, torch.int32, dev), to_device_tensor(det_dist, torch.float64, dev)
    shape = (frames.num_frames, frames.max_kpts)
    assert tuple(octave.shape) == tuple(det_dist.shape) == shape
    level = torch.zeros(shape, dtype=torch.int32, device=dev)
    torch.cuda.current_stream(dev).synchronize()
    fv = frames.view()
    _on_torch_stream(ctx, dev, lambda: ctx.frame_levels_device(fv, octave.data_ptr(), det_dist.data_ptr(), level.data_ptr()),
                     use_torch_stream)
    level.inputs = (octave, det_dist)
    return level


class PoseSetsDevice(FrameSet):
    """What ps_pose_sets_device wrote: a frame set of S + 1 frames -- set s = the features observed from poses[s], frame S the
    empty set --, set_count (S,) and the side arrays feat_idx / obs_idx (S + 1, cap) int32 (side_arrays=False: not kept, NULL is
    passed).  packed_stride: bytes per set of ONE block [cap x 32 B descriptors][cap x 12 B points] instead of two dense arrays."""

    def __init__(self, S, max_kpts, device, packed_stride=None, side_arrays=True):
        self.device = torch.device(device)
        self.S, self.num_frames, self.max_kpts = int(S), int(S) + 1, int(max_kpts)
        n, cap = self.num_frames, self.max_kpts
        new = lambda shape, dt: _zeros(self.device, shape, dt)   # noqa: E731
        self._zero_frames(n, packed_stride)
        self.set_count = new((max(self.S, 1),), torch.int32)
        self.feat_idx, self.obs_idx = (new((n, cap), torch.int32), new((n, cap), torch.int32)) if side_arrays else (None, None)
        torch.cuda.current_stream(self.device).synchronize()   # (the fills are done before a context's stream writes)

    def out_struct(self):
        side = (None, None) if self.feat_idx is None else (self.feat_idx.data_ptr(), self.obs_idx.data_ptr())
        return PsPoseSetOut(self.frame_set(), self.set_count.data_ptr(), *side)

    def download(self):
        """Everything on the host (numpy); desc (S + 1, cap, 32) and pts (S + 1, cap, 3) whatever the layout."""
        torch.cuda.synchronize(self.device)
        desc, pts = self.download_frames()
        out = dict(desc=desc, pts=pts, nkpts=self.nkpts.cpu().numpy(), setCount=self.set_count.cpu().numpy()[:self.S])
        if self.feat_idx is not None:
            out.update(featIdx=self.feat_idx.cpu().numpy(), obsIdx=self.obs_idx.cpu().numpy())
        return out


def build_pose_sets(ctx, store: MapStoreDevice, obs_point3d, poses, max_kpts, packed_stride=None, out=None, side_arrays=True,
                    use_torch_stream=True):
    """ps_pose_sets_device: the feature sets of the poses `poses` (S pose ids; numpy or a device tensor) from the resident
    store, asynchronous, ordered like `run_map_pairs`.  obs_point3d (O, 3) float64: ExtendedDescriptor::point3D of every
    observation of the store, passed beside it (numpy, or a device tensor that stays resident with the store).
    Returns a PoseSetsDevice (`out`, if given, is written again)."""
    dev = store.device
    obs_point3d = to_device_tensor(obs_point3d, torch.float64, dev, (-1, 3))
    assert tuple(obs_point3d.shape) == (store.num_obs, 3)
    poses = to_device_tensor(poses, torch.int32, dev, (-1,))
    assert poses.dim() == 1
    S = int(poses.shape[0])
    if out is None:
        out = PoseSetsDevice(S, max_kpts, dev, packed_stride, side_arrays)
    assert out.S == S and out.max_kpts == int(max_kpts)
    req = PsPoseSetRequest(obs_point3d.data_ptr() if store.num_obs else None, poses.data_ptr() if S else None, S, 0)
    torch.cuda.current_stream(dev).synchronize()   # (uploads above are complete before the context's stream reads them)
    out.inputs = (obs_point3d, poses, store)       # the request's device arrays live as long as the result
    st, os_ = store.view(), out.out_struct()
    _on_torch_stream(ctx, dev, lambda: ctx.pose_sets_device(st, req, os_), use_torch_stream)
    return out


class LoopBatchDevice(PairResultsDevice):
    """A batch of loop-closure candidates in HBM (PsLoopBatch + PsLoopResults): `sets` as build_pose_sets wrote them, pairs (L, 2)
    of SET indices ([0] the query / prev side), the two thresholds of FeaturesMap::loopClosure, and the output block."""

    def __init__(self, sets: PoseSetsDevice, pairs, min_features=35, ratio_threshold=0.4, paired_feat=True):
        self.sets = sets
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        self.L = pairs.shape[0]
        self.min_features, self.ratio_threshold = int(min_features), float(ratio_threshold)
        L, cap = max(self.L, 1), sets.max_kpts
        new = lambda shape, dt: _zeros(sets.device, shape, dt)   # noqa: E731
        self.pairs = torch.from_numpy(pairs).to(sets.device) if self.L else new((1, 2), torch.int32)
        self.ratio, self.closed, self.num_paired = new((L,), torch.float64), new((L,), torch.int32), new((L,), torch.int32)
        self.paired_rows = new((L, cap, 2), torch.int32)
        self.paired_feat = new((L, cap, 2), torch.int32) if paired_feat else None
        super().__init__(self.L, cap, sets.device)

    def batch_struct(self):
        s = self.sets
        return PsLoopBatch(s.frame_set(), s.set_count.data_ptr(), s.feat_idx.data_ptr() if s.feat_idx is not None else None,
                           self.pairs.data_ptr(), self.L, s.S, self.min_features, 0, self.ratio_threshold)

    def results_struct(self):
        return PsLoopResults(self.view().struct(), self.ratio.data_ptr(), self.closed.data_ptr(), self.num_paired.data_ptr(),
                             self.paired_rows.data_ptr(), self.paired_feat.data_ptr() if self.paired_feat is not None else None)

    def download(self):
        out, g = super().download(), (lambda t: t.cpu().numpy()[:self.L])
        out.update(ratio=g(self.ratio), closed=g(self.closed), numPaired=g(self.num_paired), pairedRows=g(self.paired_rows))
        if self.paired_feat is not None:
            out["pairedFeat"] = g(self.paired_feat)
        return out


def run_loop_pairs(ctx, params, cfg, K, batch: LoopBatchDevice, use_torch_stream=True):
    """Asynchronous: gate -> match -> RANSAC -> refit -> verdict for every candidate of the batch (ps_loop_pairs_device), ordered
    like `run_pairs`: after the work already queued on torch's current stream, which waits for the results."""
    b, r = batch.batch_struct(), batch.results_struct()
    _on_torch_stream(ctx, batch.device, lambda: ctx.loop_pairs_device(params, cfg, K, b, r), use_torch_stream)


# ---- the resident store with float descriptor rows (SURF / SIFT): ps_map_views_l2_device / ps_pose_sets_l2_device /
# ps_loop_pairs_l2_device
def _rows_f32(device, rows, dim, row_floats, offset_floats):
    """(flat, rows view): zero-filled float32 storage for `rows` rows of `dim` floats lying row_floats floats apart, the first
    one offset_floats floats behind the allocation's (256-byte aligned) base."""
    row_floats = dim if row_floats is None else int(row_floats)
    assert row_floats >= dim and offset_floats >= 0
    flat = _zeros(device, (int(offset_floats) + max(rows, 1) * row_floats,), torch.float32)
    return flat, flat[int(offset_floats):].view(max(rows, 1), row_floats), row_floats


class MapStoreF32Device:
    """MapStoreDevice with float descriptor rows (PsMapStoreF32): obs_desc (O, dim) float32.  row_floats > dim: the rows lie
    row_floats floats apart, what lies between them holds `pad` (never read by the library); offset_floats: the first row lies
    that many floats behind the allocation's base (a store that is not 16-byte aligned).  Rows are uploaded as they are: NaN
    payloads, -0.0 and subnormals included."""

    def __init__(self, pos, obs_start, obs_pose, obs_desc, obs_octave, obs_det_dist, num_poses, device="cuda:0", row_floats=None,
                 pad=np.nan, offset_floats=0):
        self.device = torch.device(device)
        pos = np.ascontiguousarray(pos, np.float64).reshape(-1, 3)
        obs_start = np.ascontiguousarray(obs_start, np.int32)
        obs_pose = np.ascontiguousarray(obs_pose, np.int32)
        obs_desc = np.ascontiguousarray(obs_desc, np.float32)
        assert obs_desc.ndim == 2
        obs_octave = np.ascontiguousarray(obs_octave, np.int32)
        obs_det_dist = np.ascontiguousarray(obs_det_dist, np.float64)
        self.num_features, self.num_obs, self.num_poses = pos.shape[0], obs_pose.shape[0], int(num_poses)
        self.dim = int(obs_desc.shape[1])
        assert obs_start.shape == (self.num_features + 1,)
        assert obs_desc.shape[0] == obs_octave.shape[0] == obs_det_dist.shape[0] == self.num_obs
        self.desc_flat, self.obs_desc, self.row_floats = _rows_f32(self.device, self.num_obs, self.dim, row_floats, offset_floats)
        if self.num_obs:
            wide = np.full((self.num_obs, self.row_floats), pad, np.float32)
            wide.view(np.uint32)[:, :self.dim] = obs_desc.view(np.uint32)   # (bit for bit)
            self.obs_desc.view(torch.int32).copy_(torch.from_numpy(wide.view(np.int32)))
        up = lambda a: torch.from_numpy(a).to(self.device)   # noqa: E731
        self.pos, self.obs_start, self.obs_pose = up(pos), up(obs_start), up(obs_pose)
        self.obs_octave, self.obs_det_dist = up(obs_octave), up(obs_det_dist)
        torch.cuda.current_stream(self.device).synchronize()   # (resident before a context's own stream reads it)

    def view(self):
        return PsMapStoreF32(self.pos.data_ptr(), self.obs_start.data_ptr(), self.obs_pose.data_ptr(), self.obs_desc.data_ptr(),
                             self.obs_octave.data_ptr(), self.obs_det_dist.data_ptr(), self.num_features, self.num_obs,
                             self.num_poses, self.dim, 0 if self.row_floats == self.dim else self.row_floats * 4)


class FrameSetF32Out:
    """A float-descriptor frame set the library writes (PsFrameSetF32): desc (n, cap, row_floats) float32 -- a view of desc_flat
    that starts offset_floats floats behind its base --, pts (n, cap, 3) float32, nkpts (n,) int32.  Usable wherever a
    FrameSetF32Device is (MapBatchF32Device.maps, run_match_l2)."""

    def _zero_frames(self, n, dim, row_floats, offset_floats):
        cap, dev = self.max_kpts, self.device
        self.dim, self.offset_floats = int(dim), int(offset_floats)
        self.desc_flat, rows, self.row_floats = _rows_f32(dev, n * cap, self.dim, row_floats, offset_floats)
        self.desc = rows.view(n, cap, self.row_floats)
        self.pts = _zeros(dev, (n, cap, 3), torch.float32)
        self.nkpts = _zeros(dev, (n,), torch.int32)

    def view(self):
        dense = self.row_floats == self.dim
        return api.DeviceFramesF32(self.desc.data_ptr(), self.pts.data_ptr(), self.nkpts.data_ptr(), self.num_frames, self.max_kpts,
                                   self.dim, 0 if dense else self.row_floats * 4, 0 if dense else self.max_kpts * self.row_floats * 4, 0)

    def frame_set(self):
        return self.view().struct()

    def download_frames(self):
        """(desc (n, cap, dim) float32, pts (n, cap, 3)) on the host; the rows bit for bit (copied as 32-bit words)."""
        d = self.desc.view(torch.int32).cpu().numpy().view(np.float32)
        return np.ascontiguousarray(d[:, :, :self.dim]), self.pts.cpu().numpy()


class MapViewsF32Device(FrameSetF32Out):
    """What ps_map_views_l2_device wrote: MapViewsDevice with float rows of `dim` floats; feeds MapBatchF32Device (maps =
    this object, map_level = .map_level).  obs_idx=False: no obsIdx array is kept (NULL is passed: the library records the rows'
    observations in its own scratch)."""

    def __init__(self, V, max_kpts, dim, device, row_floats=None, offset_floats=0, obs_idx=True):
        self.device = torch.device(device)
        self.num_frames, self.max_kpts = int(V), int(max_kpts)
        n, cap = max(self.num_frames, 1), self.max_kpts
        new = lambda shape, dt: _zeros(self.device, shape, dt)   # noqa: E731
        self._zero_frames(n, dim, row_floats, offset_floats)
        self.view_count = new((n,), torch.int32)
        self.map_level, self.feat_idx = new((n, cap), torch.int32), new((n, cap), torch.int32)
        self.obs_idx = new((n, cap), torch.int32) if obs_idx else None
        self.pos_cam, self.uv, self.angle = new((n, cap, 3), torch.float64), new((n, cap, 2), torch.float64), new((n, cap), torch.float64)
        torch.cuda.current_stream(self.device).synchronize()   # (the fills are done before a context's stream writes)

    def out_struct(self):
        return PsMapViewOutF32(self.frame_set(), self.map_level.data_ptr(), self.view_count.data_ptr(), self.feat_idx.data_ptr(),
                               self.obs_idx.data_ptr() if self.obs_idx is not None else None, self.pos_cam.data_ptr(),
                               self.uv.data_ptr(), self.angle.data_ptr())

    def download(self):
        torch.cuda.synchronize(self.device)
        V = self.num_frames
        desc, pts = self.download_frames()
        g = lambda t: t.cpu().numpy()[:V]   # noqa: E731
        out = dict(desc=desc[:V], pts=pts[:V], nkpts=g(self.nkpts), viewCount=g(self.view_count), mapLevel=g(self.map_level),
                   featIdx=g(self.feat_idx), posCam=g(self.pos_cam), uv=g(self.uv), angle=g(self.angle))
        if self.obs_idx is not None:
            out["obsIdx"] = g(self.obs_idx)
        return out


def build_map_views_l2(ctx, store: MapStoreF32Device, cam_inv, pose_angle, max_angle, K, image_size, max_kpts, cand=None,
                       cand_counts=None, require_visible=False, out=None, row_floats=None, obs_idx=True, use_torch_stream=True):
    """build_map_views for a store of float rows (ps_map_views_l2_device): the same arguments; returns a MapViewsF32Device
    (`out`, if given, is written again)."""
    dev = store.device
    req, keep, V = _map_view_request(store, cam_inv, pose_angle, max_angle, K, image_size, cand, cand_counts, require_visible)
    if out is None:
        out = MapViewsF32Device(V, max_kpts, store.dim, dev, row_floats, 0, obs_idx)
    assert out.num_frames >= V and out.max_kpts == int(max_kpts)
    torch.cuda.current_stream(dev).synchronize()   # (uploads above are complete before the context's stream reads them)
    out.inputs = keep + [store]
    st, os_ = store.view(), out.out_struct()
    _on_torch_stream(ctx, dev, lambda: ctx.map_views_l2_device(st, req, os_), use_torch_stream)
    return out


class PoseSetsF32Device(FrameSetF32Out):
    """What ps_pose_sets_l2_device wrote: PoseSetsDevice with float rows of `dim` floats (S + 1 frames, frame S the empty set)."""

    def __init__(self, S, max_kpts, dim, device, row_floats=None, offset_floats=0, side_arrays=True):
        self.device = torch.device(device)
        self.S, self.num_frames, self.max_kpts = int(S), int(S) + 1, int(max_kpts)
        n, cap = self.num_frames, self.max_kpts
        new = lambda shape, dt: _zeros(self.device, shape, dt)   # noqa: E731
        self._zero_frames(n, dim, row_floats, offset_floats)
        self.set_count = new((max(self.S, 1),), torch.int32)
        self.feat_idx, self.obs_idx = (new((n, cap), torch.int32), new((n, cap), torch.int32)) if side_arrays else (None, None)
        torch.cuda.current_stream(self.device).synchronize()   # (the fills are done before a context's stream writes)

    def out_struct(self):
        side = (None, None) if self.feat_idx is None else (self.feat_idx.data_ptr(), self.obs_idx.data_ptr())
        return PsPoseSetOutF32(self.frame_set(), self.set_count.data_ptr(), *side)

    def download(self):
        torch.cuda.synchronize(self.device)
        desc, pts = self.download_frames()
        out = dict(desc=desc, pts=pts, nkpts=self.nkpts.cpu().numpy(), setCount=self.set_count.cpu().numpy()[:self.S])
        if self.feat_idx is not None:
            out.update(featIdx=self.feat_idx.cpu().numpy(), obsIdx=self.obs_idx.cpu().numpy())
        return out


def build_pose_sets_l2(ctx, store: MapStoreF32Device, obs_point3d, poses, max_kpts, row_floats=None, out=None, side_arrays=True,
                       use_torch_stream=True):
    """build_pose_sets for a store of float rows (ps_pose_sets_l2_device); returns a PoseSetsF32Device."""
    dev = store.device
    obs_point3d = to_device_tensor(obs_point3d, torch.float64, dev, (-1, 3))
    assert tuple(obs_point3d.shape) == (store.num_obs, 3)
    poses = to_device_tensor(poses, torch.int32, dev, (-1,))
    assert poses.dim() == 1
    S = int(poses.shape[0])
    if out is None:
        out = PoseSetsF32Device(S, max_kpts, store.dim, dev, row_floats, 0, side_arrays)
    assert out.S == S and out.max_kpts == int(max_kpts)
    req = PsPoseSetRequest(obs_point3d.data_ptr() if store.num_obs else None, poses.data_ptr() if S else None, S, 0)
    torch.cuda.current_stream(dev).synchronize()   # (uploads above are complete before the context's stream reads them)
    out.inputs = (obs_point3d, poses, store)
    st, os_ = store.view(), out.out_struct()
    _on_torch_stream(ctx, dev, lambda: ctx.pose_sets_l2_device(st, req, os_), use_torch_stream)
    return out


class LoopBatchF32Device(LoopBatchDevice):
    """LoopBatchDevice for float-descriptor sets (PsLoopBatchF32): `sets` as build_pose_sets_l2 wrote them."""

    def batch_struct(self):
        s = self.sets
        return PsLoopBatchF32(s.frame_set(), s.set_count.data_ptr(), s.feat_idx.data_ptr() if s.feat_idx is not None else None,
                              self.pairs.data_ptr(), self.L, s.S, self.min_features, 0, self.ratio_threshold)


def run_loop_pairs_l2(ctx, params, cfg, K, batch: LoopBatchF32Device, use_torch_stream=True):
    """run_loop_pairs for float descriptors (ps_loop_pairs_l2_device)."""
    b, r = batch.batch_struct(), batch.results_struct()
    _on_torch_stream(ctx, batch.device, lambda: ctx.loop_pairs_l2_device(params, cfg, K, b, r), use_torch_stream)
