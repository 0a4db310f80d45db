"""LPIPS (VGG-16 variant, v0.1) of predicted clips on the MI355X: libivg ``ivg_lpips_rows`` (csrc/lpips.hip).  The fourth metric of the
reference's ``Evaluator.forward`` (ivideogpt/utils/video_metric.py:75-88).  The weights are the caller's -- torchvision's ``vgg16``
features plus the ``lpips`` package's ``vgg.pth`` linear layers, or a state dict of the reference's own LPIPS class
(ivideogpt/vq_model/lpips.py); none ship here.  No compute in Python: this module maps names, packs layouts and allocates buffers."""
import ctypes as C

import torch

from . import _lib
from .packing import dtype_code, pack_lpips


def _load_file(path):
    if str(path).endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(str(path))
    sd = torch.load(str(path), map_location="cpu", weights_only=True)
    return sd.get("state_dict", sd) if isinstance(sd, dict) else sd


class LPIPS:
    """``LPIPS.from_state_dict(sd).to("cuda")(gt, pred) -> rows (B,)``: gt (B, T, 3, H, W) float32 / bfloat16 in [0, 1], pred float32
    (t * B, T', 3, H, W) with sample k of trajectory b at row k * B + b; per frame pair the LPIPS distance, mean over the compared
    frames of a trajectory, min over its t samples.  ``max_images``: images per pass through the network (bounds the scratch; the
    result does not depend on it)."""

    def __init__(self, packed, max_images=None):
        self._cpu = packed               # canonical names -> packed fp32 CPU tensors
        self.max_images = max_images
        self.device = None
        self._w = self._handle = None
        self._ws = {}                    # stream handle -> scratch tensor

    @classmethod
    def from_state_dict(cls, sd, max_images=None):
        return cls(pack_lpips(sd), max_images)

    @classmethod
    def from_files(cls, vgg16_features_path, lin_path, max_images=None):
        sd = dict(_load_file(vgg16_features_path))
        sd.update(_load_file(lin_path))
        return cls(pack_lpips(sd), max_images)

    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("LPIPS runs on the MI355X only (no CPU path)")
        device = torch.device("cuda", torch.cuda.current_device() if device.index is None else device.index)
        if self._handle is not None and device == self.device:
            return self
        self._release()
        self._w = {k: v.to(device).contiguous() for k, v in self._cpu.items()}
        names = [k.encode() for k in self._w]
        table = (_lib.IvgTensor * len(names))()
        for i, (k, v) in enumerate(self._w.items()):
            table[i].name, table[i].data, table[i].dtype, table[i].ndim = names[i], v.data_ptr(), _lib.IVG_F32, v.dim()
            for d, s in enumerate(v.shape):
                table[i].shape[d] = s
        h = C.c_void_p()
        _lib.check(_lib.load().ivg_lpips_create(table, len(names), device.index, C.byref(h)), None, "lpips_create")
        self._handle, self.device = h, device
        self._ws = {}
        return self

    def _release(self):
        if self._handle is not None:
            _lib.load().ivg_lpips_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    @torch.no_grad()
    def frames_and_rows(self, video_gt, video_pred, gt_t0=0, pred_t0=0, frames=None, max_images=None):
        """-> (per-frame values float32 (t * B, T), rows float32 (B,))"""
        if self._handle is None:
            if not video_gt.is_cuda:
                raise RuntimeError("LPIPS runs on the MI355X only (no CPU path)")
            self.to(video_gt.device)
        lib = _lib.load()
        gt = video_gt if video_gt.dtype in (torch.float32, torch.bfloat16) else video_gt.float()
        gt, pred = gt.to(self.device).contiguous(), video_pred.to(self.device).float().contiguous()
        B, Tg, _, H, W = gt.shape
        n, Tp = pred.shape[:2]
        T = frames if frames is not None else min(Tg - gt_t0, Tp - pred_t0)
        t = max(1, n // B)
        cap = max_images if max_images is not None else self.max_images
        images = B * T * (1 + t) if cap is None else max(2, min(int(cap), B * T * (1 + t)))
        nbytes = lib.ivg_lpips_ws_bytes(images, H, W)
        stream = torch.cuda.current_stream(self.device)
        ws = self._ws.get(stream.cuda_stream)
        if ws is None or ws.numel() < nbytes:
            self._ws.pop(stream.cuda_stream, None)
            ws = self._ws[stream.cuda_stream] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        per_frame = torch.empty(n, T, dtype=torch.float32, device=self.device)
        rows = torch.empty(B, dtype=torch.float32, device=self.device)
        P = lambda x: C.c_void_p(x.data_ptr())
        _lib.check(lib.ivg_lpips_rows(self._handle, P(gt), dtype_code(gt.dtype), B, Tg, gt_t0, P(pred), n, Tp, pred_t0, T, H, W, P(per_frame), P(rows),
                                      P(ws), nbytes, C.c_void_p(stream.cuda_stream)), None, "lpips_rows")
        return per_frame, rows

    def __call__(self, video_gt, video_pred, **kw):
        return self.frames_and_rows(video_gt, video_pred, **kw)[1]

    def frames(self, video_gt, video_pred, **kw):
        return self.frames_and_rows(video_gt, video_pred, **kw)[0]
