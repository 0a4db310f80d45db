"""Kinetics-400 Inception-I3D features of clips on the MI355X: libivg ``ivg_i3d_features`` (csrc/i3d.hip), the detector behind the
reference's FVD (ivideogpt/utils/video_metric.py:26-55: a torchscript file called with ``rescale=True, resize=True,
return_features=True``).  The weights are the caller's -- the state dict of that torchscript file, or of the public PyTorch port of
Kinetics I3D; none ship here.  No compute in Python: this module maps names, packs layouts and allocates buffers."""
import ctypes as C

import torch

from . import _lib
from .packing import dtype_code, pack_i3d

DEFAULT_MAX_CLIPS = 8   # clips per pass through the trunk when the caller sets no bound (about 0.1 GB of scratch per 16 x 224 x 224 clip)


def min_frames():
    """the shortest clip that leaves two time steps in front of the average pool (three stride-2 stages: ceil(T / 8) >= 2)"""
    return 9


class I3D:
    """``I3D.from_state_dict(sd).to("cuda").features(video) -> (B, 400)`` float32: video (B, T, 3, H, W) float32 / bfloat16 in
    [0, 1]; every frame is resized to ``resize`` x ``resize`` (bilinear, a multiple of 32), mapped to 2 x - 1, and the clip goes through the
    trunk; the features are the pre-softmax logits averaged over the remaining time steps.  ``max_clips``: clips per pass (bounds the
    scratch; the result does not depend on it)."""

    def __init__(self, packed, resize=224, max_clips=None):
        if resize <= 0 or resize % 32:
            raise ValueError(f"I3D: resize {resize} is not a positive multiple of 32")
        self._cpu = packed
        self.resize, self.max_clips = int(resize), max_clips
        self.num_features = packed["logits.weight"].shape[0]
        self.device = None
        self._w = self._handle = None
        self._ws = {}

    @classmethod
    def from_state_dict(cls, sd, resize=224, max_clips=None):
        return cls(pack_i3d(sd), resize, max_clips)

    @classmethod
    def from_torchscript(cls, path, resize=224, max_clips=None):
        """the state dict of the torchscript detector file; nothing of the script is executed"""
        return cls.from_state_dict(torch.jit.load(str(path), map_location="cpu").state_dict(), resize, max_clips)

    @classmethod
    def from_file(cls, path, resize=224, max_clips=None):
        """a torchscript archive or a plain state-dict file (``torch.save`` / safetensors)"""
        if str(path).endswith(".safetensors"):
            from safetensors.torch import load_file
            return cls.from_state_dict(load_file(str(path)), resize, max_clips)
        try:
            sd = torch.load(str(path), map_location="cpu", weights_only=True)
        except Exception:
            return cls.from_torchscript(path, resize, max_clips)
        if hasattr(sd, "state_dict"):
            sd = sd.state_dict()
        return cls.from_state_dict(sd.get("state_dict", sd), resize, max_clips)

    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("I3D runs on the MI355X only (no CPU path)")
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
        _lib.check(_lib.load().ivg_i3d_create(table, len(names), device.index, self.resize, C.byref(h)), None, "i3d_create")
        self._handle, self.device = h, device
        self._ws = {}
        return self

    def _release(self):
        if self._handle is not None:
            _lib.load().ivg_i3d_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def _scratch(self, clips, T, H, W):
        nbytes = _lib.load().ivg_i3d_ws_bytes(self._handle, clips, T, H, W)
        stream = torch.cuda.current_stream(self.device)
        ws = self._ws.get(stream.cuda_stream)
        if ws is None or ws.numel() < nbytes:
            self._ws.pop(stream.cuda_stream, None)
            ws = self._ws[stream.cuda_stream] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return ws, nbytes, stream

    def _prepare(self, video, max_clips):
        if self._handle is None:
            if not video.is_cuda:
                raise RuntimeError("I3D runs on the MI355X only (no CPU path)")
            self.to(video.device)
        if video.dim() != 5 or video.shape[2] != 3:
            raise ValueError(f"I3D: expected clips (B, T, 3, H, W), got {tuple(video.shape)}")
        if video.shape[1] < min_frames():
            raise ValueError(f"I3D: {video.shape[1]} frames leave fewer than two time steps in front of the average pool (at least {min_frames()})")
        v = video if video.dtype in (torch.float32, torch.bfloat16) else video.float()
        v = v.to(self.device).contiguous()
        cap = max_clips if max_clips is not None else (self.max_clips if self.max_clips is not None else DEFAULT_MAX_CLIPS)
        return v, max(1, min(int(cap), v.shape[0]))

    @torch.no_grad()
    def features(self, video, max_clips=None):
        v, clips = self._prepare(video, max_clips)
        B, T, _, H, W = v.shape
        ws, nbytes, stream = self._scratch(clips, T, H, W)
        out = torch.empty(B, self.num_features, dtype=torch.float32, device=self.device)
        P = lambda x: C.c_void_p(x.data_ptr())
        _lib.check(_lib.load().ivg_i3d_features(self._handle, P(v), dtype_code(v.dtype), B, T, H, W, P(out), P(ws), nbytes,
                                                C.c_void_p(stream.cuda_stream)), None, "i3d_features")
        return out

    __call__ = features

    @torch.no_grad()
    def tap(self, video, unit, max_clips=None):
        """test hook (``ivg_op_i3d_tap``): -> (activation (B, D, H, W, C) after unit ``unit`` of a forward, the units it reads)"""
        v, clips = self._prepare(video, max_clips)
        B, T, _, H, W = v.shape
        lib = _lib.load()
        dims = (C.c_int64 * 8)()
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(lib.ivg_op_i3d_tap(self._handle, None, dtype_code(v.dtype), B, T, H, W, unit, None, dims, None, 0, st), None, "i3d_tap")
        ws, nbytes, stream = self._scratch(clips, T, H, W)
        out = torch.empty(B, *dims[:4], dtype=torch.float32, device=self.device)
        P = lambda x: C.c_void_p(x.data_ptr())
        _lib.check(lib.ivg_op_i3d_tap(self._handle, P(v), dtype_code(v.dtype), B, T, H, W, unit, P(out), dims, P(ws), nbytes,
                                      C.c_void_p(stream.cuda_stream)), None, "i3d_tap")
        return out, [s for s in dims[4:8] if s != -2]

    def num_units(self):
        return _lib.load().ivg_i3d_units(self._handle)
