"""Frame metrics of predicted clips on the MI355X (libivg ``ivg_frame_metrics``): the reference's ``Evaluator.forward``
(/root/reference/ivideogpt/utils/video_metric.py:63-100): per-frame MSE, PSNR and SSIM (piqa semantics), mean over a
trajectory's frames, best of the ``t`` samples drawn per trajectory; LPIPS the same way when the caller supplies the network
weights (``Evaluator(lpips=...)``, ivideogpt_amd/lpips.py).  FVD (:26-55, :103-173) when the caller supplies the I3D detector
(``Evaluator(i3d=...)``, ivideogpt_amd/i3d.py): features on the device, ``FeatureStats`` and ``frechet_distance`` on the host in fp64."""
import ctypes as C
import threading

import torch

from . import _lib
from .packing import dtype_code


_WS = {}   # (device, stream) -> scratch tensor of ivg_frame_metrics (partial sums of the metric tiles), least recently used first
_WS_MAX = 16   # a raw stream handle can be reused by a NEW stream after the old one died: a bounded cache also bounds how long such a
               # stale association lives (the buffer is private to one call's kernels either way -- ordered by the stream it runs on)
_WS_LOCK = threading.Lock()   # the lanes' host threads (bench.py --lanes) all come through here: pop / insert / evict as one step


@torch.no_grad()
def frame_metric_rows(video_gt, video_pred, gt_t0=0, pred_t0=0, frames=None):
    """video_gt (B, T, 3, H, W) float32 / bfloat16 on the GPU; video_pred float32 (t * B, T', 3, H, W), sample k of trajectory b
    at row k * B + b.  Frames [gt_t0, gt_t0 + frames) of the ground truth are compared with [pred_t0, pred_t0 + frames) of the
    prediction (default: everything after the offsets).  -> float32 (B, 3) rows (mse, psnr, ssim), best of t per trajectory."""
    lib = _lib.load()
    if not video_gt.is_cuda:
        raise RuntimeError("frame metrics run on the MI355X only (no CPU path)")
    gt = video_gt if video_gt.dtype in (torch.float32, torch.bfloat16) else video_gt.float()
    gt, pred = gt.contiguous(), video_pred.float().contiguous()
    B, Tg, _, H, W = gt.shape
    n, Tp = pred.shape[:2]
    T = frames if frames is not None else min(Tg - gt_t0, Tp - pred_t0)
    rows = torch.empty(B, 3, dtype=torch.float32, device=gt.device)
    nbytes = lib.ivg_frame_metrics_ws_bytes(n, T, H, W)
    # The scratch is kept PER (device, stream): no allocation on the hot path (a serving loop calls this every step), and two batches
    # in flight on two streams / host threads (bench.py --lanes) never share partial sums -- the tile kernel writes them and the reduce
    # kernel of the same call reads them back, ordered by the stream.  A buffer that has to grow is replaced by one allocated under
    # the same current stream, so the caching allocator hands the old block only to later work of that stream.
    stream = torch.cuda.current_stream(gt.device)
    key = (gt.device, stream.cuda_stream)
    with _WS_LOCK:
        ws = _WS.pop(key, None)           # (re-inserted below: the dict is in least-recently-used order)
        if ws is None or ws.numel() * 4 < nbytes:
            ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=gt.device)
        _WS[key] = ws
        while len(_WS) > _WS_MAX:         # callers that keep creating streams (CU-masked ExternalStreams, short-lived lanes) do not leak
            _WS.pop(next(iter(_WS)))      # one buffer per dead handle; an evicted buffer's block returns to the caching allocator
    st = C.c_void_p(stream.cuda_stream)
    _lib.check(lib.ivg_frame_metrics(C.c_void_p(gt.data_ptr()), dtype_code(gt.dtype), B, Tg, gt_t0, C.c_void_p(pred.data_ptr()), n, Tp, pred_t0,
                                     T, H, W, C.c_void_p(rows.data_ptr()), C.c_void_p(ws.data_ptr()), nbytes, st), None, "frame_metrics")
    return rows


class FeatureStats:
    """The reference's ``FeatureStats(capture_mean_cov=True)`` (ivideogpt/utils/video_metric.py:118-173): running fp64 sum and
    X^T X of float32 feature rows on the host; ``get_mean_cov`` returns the mean and the BIASED covariance (divided by N)."""

    def __init__(self, capture_all=False, capture_mean_cov=True, max_items=None):
        self.capture_all, self.capture_mean_cov, self.max_items = capture_all, capture_mean_cov, max_items
        self.num_items, self.num_features = 0, None
        self.all_features = self.raw_mean = self.raw_cov = None

    def set_num_features(self, num_features):
        if self.num_features is not None:
            assert num_features == self.num_features
            return
        import numpy as np
        self.num_features, self.all_features = num_features, []
        self.raw_mean = np.zeros([num_features], dtype=np.float64)
        self.raw_cov = np.zeros([num_features, num_features], dtype=np.float64)

    def is_full(self):
        return self.max_items is not None and self.num_items >= self.max_items

    def append(self, x):
        import numpy as np
        x = np.asarray(x, dtype=np.float32)
        assert x.ndim == 2
        if self.max_items is not None and self.num_items + x.shape[0] > self.max_items:
            if self.num_items >= self.max_items:
                return
            x = x[:self.max_items - self.num_items]
        self.set_num_features(x.shape[1])
        self.num_items += x.shape[0]
        if self.capture_all:
            self.all_features.append(x)
        if self.capture_mean_cov:
            x64 = x.astype(np.float64)
            self.raw_mean += x64.sum(axis=0)
            self.raw_cov += x64.T @ x64

    def append_torch(self, x):
        self.append(x.detach().float().cpu().numpy())

    def get_all(self):
        import numpy as np
        assert self.capture_all
        return np.concatenate(self.all_features, axis=0)

    def get_mean_cov(self):
        import numpy as np
        assert self.capture_mean_cov
        mean = self.raw_mean / self.num_items
        return mean, self.raw_cov / self.num_items - np.outer(mean, mean)


def _trace_sqrt_product(sigma_g, sigma_r, method):
    """tr sqrtm(sigma_g sigma_r): ``scipy.linalg.sqrtm`` as the reference, or -- the product of two covariance matrices has real
    non-negative eigenvalues, and the trace of the principal square root is the sum of their square roots -- the real parts of the
    complex square roots of ``eigvals``."""
    import numpy as np
    prod = np.dot(sigma_g, sigma_r)
    if method is None:
        try:
            import scipy.linalg  # noqa: F401
            method = "scipy"
        except Exception:
            method = "eig"
    if method == "scipy":
        import scipy.linalg
        try:
            s = scipy.linalg.sqrtm(prod, disp=False)
        except TypeError:
            s = scipy.linalg.sqrtm(prod)
        s = s[0] if isinstance(s, tuple) else s
        return float(np.real(np.trace(s)))
    if method != "eig":
        raise ValueError(f"frechet_distance: unknown method {method!r}")
    return float(np.sqrt(np.linalg.eigvals(prod).astype(np.complex128)).real.sum())


def frechet_distance(mu_g, sigma_g, mu_r, sigma_r, method=None):
    """|mu_g - mu_r|^2 + tr(sigma_g + sigma_r - 2 sqrtm(sigma_g sigma_r)) on the host in fp64, as the reference's ``compute_fvd``
    (video_metric.py:29-39).  ``method``: "scipy", "eig", or None = scipy where it imports."""
    import numpy as np
    mu_g, mu_r = np.asarray(mu_g, dtype=np.float64), np.asarray(mu_r, dtype=np.float64)
    sigma_g, sigma_r = np.asarray(sigma_g, dtype=np.float64), np.asarray(sigma_r, dtype=np.float64)
    m = np.square(mu_g - mu_r).sum()
    return float(m + np.trace(sigma_g) + np.trace(sigma_r) - 2.0 * _trace_sqrt_product(sigma_g, sigma_r, method))


class Evaluator:
    """``Evaluator(video_1, video_2)`` of the reference's eval loop (train_gpt.py:469-472; ivideogpt/utils/video_metric.py:63-100):
    video_1 = ground truth (B, T, 3, H, W), video_2 = predictions (t * B, T, 3, H, W), sample k of trajectory b at row k * B + b.
    -> ``(mse, psnr, ssim, lpips)`` scalars like the reference's 4-tuple: per-frame metrics, mean over a trajectory's frames, best of
    its t samples (min mse, max psnr / ssim, min lpips), mean over trajectories -- computed by libivg ``ivg_frame_metrics`` and
    ``ivg_lpips_rows``.  LPIPS needs network weights that do not ship with the reference: ``lpips=`` takes an
    ``ivideogpt_amd.lpips.LPIPS`` or the pair ``(vgg16_features_path, lin_path)``; ``max_batchsize`` then bounds the images per pass
    through the network, as in the reference.  Without ``lpips=`` the fourth value is NaN: a caller that unpacks four values keeps
    working and sees an explicit not-a-number instead of a silently missing metric.  FVD needs the I3D detector's weights, which do
    not ship either: ``i3d=`` takes an ``ivideogpt_amd.i3d.I3D`` or the path of the torchscript / state-dict file (``i3d_path``, the
    reference's first argument, counts when ``i3d`` is None and the file exists); then ``i3d_features``, ``compute_fvd`` and
    ``compute_fvd_from_raw_data`` work as in the reference, without it they raise ``RuntimeError``.
    ``rows(video_1, video_2)`` returns the per-trajectory (B, 3) rows -- the payload of the multi-GPU all-gather; ``rows4`` the
    (B, 4) rows with LPIPS (needs ``lpips=``)."""

    def __init__(self, i3d_path=None, max_batchsize=None, lpips=None, i3d=None):
        self.i3d_path, self.max_batchsize = i3d_path, max_batchsize
        if lpips is not None and not hasattr(lpips, "frames_and_rows"):
            from .lpips import LPIPS
            vgg_path, lin_path = lpips
            lpips = LPIPS.from_files(vgg_path, lin_path)
        self.lpips = lpips
        # FVD detector: an ivideogpt_amd.i3d.I3D (anything with .features), or the path of the torchscript file / a state-dict file;
        # i3d_path (the reference's first argument, whose default names a file that does not ship) counts only when it exists
        import os
        if i3d is None and i3d_path is not None and os.path.isfile(str(i3d_path)):
            i3d = i3d_path
        if i3d is not None and not hasattr(i3d, "features"):
            from .i3d import I3D
            i3d = I3D.from_file(i3d)
        self.i3d = i3d

    def i3d_features(self, video):
        """video (B, T, 3, H, W) in [0, 1] -> (B, 400) float32 detector features (the reference's
        ``i3d_model(video.permute(0, 2, 1, 3, 4) * 255., rescale=True, resize=True, return_features=True)``)"""
        if self.i3d is None:
            raise RuntimeError("Evaluator was built without an I3D detector (i3d=)")
        return self.i3d.features(video, max_clips=self.max_batchsize)

    def compute_fvd(self, real_feature, gen_feature):
        """video_metric.py:29-39: the Frechet distance of two ``FeatureStats`` (``frechet_distance`` is the detector-free form)"""
        if self.i3d is None:
            raise RuntimeError("Evaluator was built without an I3D detector (i3d=)")
        if real_feature.num_items == 0 or gen_feature.num_items == 0:
            raise ValueError("No data to compute FVD")
        mu_r, sigma_r = real_feature.get_mean_cov()
        mu_g, sigma_g = gen_feature.get_mean_cov()
        return frechet_distance(mu_g, sigma_g, mu_r, sigma_r)

    def compute_fvd_from_raw_data(self, real_data=None, gen_data=None):
        """video_metric.py:41-55: ``real_data`` / ``gen_data`` (n_batches, B, T, 3, H, W) in [0, 1]; batch by batch through the detector"""
        stats = []
        for data in (real_data, gen_data):
            s = FeatureStats(capture_mean_cov=True)
            for i in range(data.shape[0]):
                clips = data[i]
                if clips.shape[2] == 1:
                    clips = clips.repeat(1, 1, 3, 1, 1)
                s.append_torch(self.i3d_features(clips))
            stats.append(s)
        return self.compute_fvd(stats[0], stats[1])

    def rows(self, video_1, video_2):
        return frame_metric_rows(video_1, video_2)

    def lpips_rows(self, video_1, video_2):
        if self.lpips is None:
            raise RuntimeError("Evaluator was built without LPIPS weights (lpips=)")
        cap = None if self.max_batchsize is None else max(2, 2 * int(self.max_batchsize))   # max_batchsize counts image PAIRS there
        return self.lpips(video_1, video_2, max_images=cap)

    def rows4(self, video_1, video_2):
        return torch.cat([self.rows(video_1, video_2), self.lpips_rows(video_1, video_2)[:, None]], 1)

    def __call__(self, video_1, video_2):
        m = self.rows(video_1, video_2).mean(0)
        if self.lpips is None:
            return m[0], m[1], m[2], torch.full((), float("nan"), device=m.device)
        return m[0], m[1], m[2], self.lpips_rows(video_1, video_2).mean()

    forward = __call__

    def eval(self):
        return self

    def to(self, *a, **k):
        return self
