"""LPIPS (include/mi_nerf_lpips.h has the definition) on the device: the fourth number of the reference's test() (utils.py:31-34, test.py:75).

``Lpips`` keeps a network plan, its packed weight blob and the scratch on the device.  The weights are data the caller supplies, like a
checkpoint: ``Lpips.from_state_dicts`` takes a VGG-16 state dict in torchvision's key names and the five linear layers of the ``lpips``
package; ``Lpips.from_arrays`` takes any plan.  Agreement with the package the reference imports (IQA_pytorch.LPIPSvgg) is NOT verified:
neither that package nor trained weights were available where this was written.  There is no fallback: every convolution runs in
libmi_nerf_lpips.so.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lpips
from ._lib import MiNerfError, dev_ptr, stream_ptr

VGG16_CONV_KEYS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)     # torchvision.models.vgg16().features indices of the 13 convolutions
# input="imagenet": torchvision's normalisation.  input="lpips": the package's 2x - 1 followed by its shift / scale, composed into one affine.
_IMAGENET_MEAN, _IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
_LPIPS_SHIFT, _LPIPS_SCALE = (-0.030, -0.088, -0.188), (0.458, 0.448, 0.450)


def input_affine(kind: str) -> Tuple[np.ndarray, np.ndarray]:
    """(a, b) of x' = a * x + b for images in [0, 1], float64."""
    if kind == "imagenet":
        mean, std = np.array(_IMAGENET_MEAN, np.float64), np.array(_IMAGENET_STD, np.float64)
        a, b = 1.0 / std, -mean / std
    elif kind == "lpips":
        shift, scale = np.array(_LPIPS_SHIFT, np.float64), np.array(_LPIPS_SCALE, np.float64)
        a, b = 2.0 / scale, (-1.0 - shift) / scale
    else:
        raise ValueError(f"input must be 'imagenet' or 'lpips', got {kind!r}")
    return a, b                                                 # float64: the packer rounds to fp32 once


def _f32(x, name: str, shape: Optional[Tuple[int, ...]] = None, numel: Optional[int] = None) -> np.ndarray:
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    if shape is not None and tuple(a.shape) != shape:
        raise ValueError(f"{name}: shape {tuple(a.shape)}, expected {shape}")
    if numel is not None and a.size != numel:
        raise ValueError(f"{name}: {a.size} values (shape {tuple(a.shape)}), expected {numel}")
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1)


def _guard(device):
    device = torch.device(device)
    if device.type != "cuda":
        raise MiNerfError(f"tensors must live on a HIP device (got {device}); this path has no CPU fallback")
    return torch.cuda.device(device)


class Lpips:
    """A packed LPIPS network.  ``model(pred, target)`` is a [n] device tensor of distances, never synchronised."""

    def __init__(self, net: _lpips.Net, blob_host: np.ndarray, device=None):
        self.net = net
        self.blob_host = blob_host                                  # uint8, mi_lpips_packed_bytes(net) long
        self.convs, self.tap_channels, self.tap_pools = _lpips.describe(net)
        self._blob: Dict[torch.device, torch.Tensor] = {}
        self._scratch: Dict[Tuple[torch.device, int, int], torch.Tensor] = {}
        if device is not None:
            self._blob_on(torch.device(device))

    # ---- construction --------------------------------------------------------------------------------
    @classmethod
    def from_arrays(cls, net, conv_w: Sequence, conv_b: Sequence, tap_w: Sequence, a, b, device=None) -> "Lpips":
        """Any plan: ``net`` a ``_lpips.Net`` (or a (cin0, ops) pair for ``_lpips.make_net``), convolution i's weight [cout, cin, 3, 3] and bias
        [cout], tap t's channel weights (any shape with C_t values), the input affine a, b [cin0]."""
        if not isinstance(net, _lpips.Net):
            net = _lpips.make_net(*net)
        L = _lpips.lib()
        nbytes = L.mi_lpips_packed_bytes(C.byref(net))
        if nbytes == 0:
            raise MiNerfError(f"mi_lpips_packed_bytes refused the network: {_lpips.last_error()}")
        convs, taps, _ = _lpips.describe(net)
        if len(conv_w) != len(convs) or len(conv_b) != len(convs) or len(tap_w) != len(taps):
            raise ValueError(f"the plan has {len(convs)} convolutions and {len(taps)} taps; got {len(conv_w)} weights, {len(conv_b)} biases, {len(tap_w)} tap weights")
        ws = [_f32(w, f"conv_w[{i}]", (co, ci, 3, 3)) for i, (w, (ci, co)) in enumerate(zip(conv_w, convs))]
        bs = [_f32(v, f"conv_b[{i}]", (co,)) for i, (v, (_, co)) in enumerate(zip(conv_b, convs))]
        ts = [_f32(v, f"tap_w[{t}]", numel=c) for t, (v, c) in enumerate(zip(tap_w, taps))]
        av, bv = _f32(a, "a", (net.cin0,)), _f32(b, "b", (net.cin0,))

        def ptrs(arrs: List[np.ndarray]):
            return (C.c_void_p * len(arrs))(*[x.ctypes.data for x in arrs])
        blob = np.empty(nbytes, np.uint8)
        _lpips.check(L.mi_lpips_pack_weights(C.byref(net), ptrs(ws), ptrs(bs), ptrs(ts), av.ctypes.data, bv.ctypes.data, blob.ctypes.data, nbytes),
                     "mi_lpips_pack_weights")
        return cls(net, blob, device)

    @classmethod
    def from_state_dicts(cls, vgg_sd, lin_sd, input: str = "imagenet", device=None) -> "Lpips":
        """VGG-16: ``vgg_sd`` in torchvision's key names (``features.N.weight`` / ``.bias`` for N in VGG16_CONV_KEYS; the same keys without
        ``features.`` are accepted), ``lin_sd`` the ``lpips`` package's ``lin{0..4}.model.1.weight`` ([1, C, 1, 1]) or a plain list of five
        tensors with C values each.  ``input``: "imagenet" or "lpips" (``input_affine``).  A missing or mis-shaped key raises ValueError
        naming it."""
        a, b = input_affine(input)
        net = _lpips.vgg16()
        convs, taps, _ = _lpips.describe(net)
        conv_w, conv_b = [], []
        for n, (ci, co) in zip(VGG16_CONV_KEYS, convs):
            for kind, shape, dst in (("weight", (co, ci, 3, 3), conv_w), ("bias", (co,), conv_b)):
                key = f"features.{n}.{kind}"
                v = vgg_sd[key] if key in vgg_sd else vgg_sd.get(f"{n}.{kind}")
                if v is None:
                    raise ValueError(f"vgg state dict: missing key {key!r} (or '{n}.{kind}')")
                if tuple(v.shape) != shape:
                    raise ValueError(f"vgg state dict: {key!r} has shape {tuple(v.shape)}, expected {shape}")
                dst.append(v)
        tap_w = []
        if isinstance(lin_sd, dict):
            for t, c in enumerate(taps):
                key = f"lin{t}.model.1.weight"
                if key not in lin_sd:
                    raise ValueError(f"lin state dict: missing key {key!r}")
                if int(np.prod(tuple(lin_sd[key].shape))) != c:
                    raise ValueError(f"lin state dict: {key!r} has shape {tuple(lin_sd[key].shape)}, expected (1, {c}, 1, 1)")
                tap_w.append(lin_sd[key])
        else:
            tap_w = list(lin_sd)
            if len(tap_w) != len(taps):
                raise ValueError(f"lin: {len(tap_w)} tensors, expected {len(taps)}")
            for t, c in enumerate(taps):
                if int(np.prod(tuple(tap_w[t].shape))) != c:
                    raise ValueError(f"lin[{t}] has shape {tuple(tap_w[t].shape)}, expected {c} values")
        return cls.from_arrays(net, conv_w, conv_b, tap_w, a, b, device)

    # ---- device state -----------------------------------------------------------------------------------
    def _blob_on(self, dev: torch.device) -> torch.Tensor:
        dev = torch.device(dev)
        if dev not in self._blob:
            self._blob[dev] = torch.from_numpy(self.blob_host).to(dev)
        return self._blob[dev]

    def _scratch_on(self, dev: torch.device, H: int, W: int) -> torch.Tensor:
        key = (torch.device(dev), H, W)
        if key not in self._scratch:
            nbytes = _lpips.lib().mi_lpips_scratch_bytes(C.byref(self.net), H, W)
            if nbytes == 0:
                raise MiNerfError(f"mi_lpips_scratch_bytes refused: {_lpips.last_error()}")
            self._scratch = {key: torch.empty(nbytes, dtype=torch.uint8, device=dev)}      # one shape at a time: a frame size change frees the old one
        return self._scratch[key]

    def _shape(self, shape, hw, what: str) -> Tuple[int, int, int]:
        c = self.net.cin0
        if len(shape) == 2 and shape[1] == c and hw is not None and int(hw[0]) * int(hw[1]) == shape[0]:
            return 1, int(hw[0]), int(hw[1])
        if len(shape) == 3 and shape[2] == c and hw is None:
            return 1, shape[0], shape[1]
        if len(shape) == 4 and shape[3] == c and hw is None:
            return shape[0], shape[1], shape[2]
        raise MiNerfError(f"{what} takes [H,W,{c}], [H*W,{c}] with hw=(H,W), or [N,H,W,{c}]; got {tuple(shape)} with hw={hw}")

    # ---- the two entries ----------------------------------------------------------------------------------
    def __call__(self, pred: torch.Tensor, target: torch.Tensor, hw=None, per_tap: bool = False):
        """LPIPS of ``pred`` against ``target``: [H,W,3], [H*W,3] with ``hw=(H,W)`` (the flat frames test() holds) or [N,H,W,3].  Returns a [N]
        device tensor; with ``per_tap`` also the [N, n_taps] terms d_t."""
        if pred.shape != target.shape or pred.numel() == 0:
            raise MiNerfError(f"pred {tuple(pred.shape)} and target {tuple(target.shape)} must match and be non-empty")
        n, H, W = self._shape(tuple(pred.shape), hw, "lpips")
        dev = pred.device
        with _guard(dev):
            p, t = dev_ptr(pred, "pred"), dev_ptr(target, "target")
            blob, scratch = self._blob_on(dev), self._scratch_on(dev, H, W)
            out = torch.empty(n, dtype=torch.float32, device=dev)
            taps = torch.empty(n, len(self.tap_channels), dtype=torch.float32, device=dev) if per_tap else None
            _lpips.check(_lpips.lib().mi_lpips_distance(C.byref(self.net), dev_ptr(blob, "blob", torch.uint8, 256), blob.numel(), p, t, n, H, W,
                                                        dev_ptr(out), dev_ptr(taps, "per_tap"), dev_ptr(scratch, "scratch", torch.uint8, 256),
                                                        scratch.numel(), stream_ptr(dev)), "mi_lpips_distance")
        return (out, taps) if per_tap else out

    def features(self, img: torch.Tensor, tap: int, hw=None) -> torch.Tensor:
        """The un-normalised features at tap ``tap`` of [H,W,3], [H*W,3] with ``hw``, or [N,H,W,3] images: [N, H_t, W_t, C_t]."""
        n, H, W = self._shape(tuple(img.shape), hw, "features")
        if not 0 <= int(tap) < len(self.tap_channels):
            raise MiNerfError(f"tap={tap} outside 0..{len(self.tap_channels) - 1}")
        dev = img.device
        with _guard(dev):
            p = dev_ptr(img, "img")
            blob, scratch = self._blob_on(dev), self._scratch_on(dev, H, W)
            s = self.tap_pools[tap]
            out = torch.empty(n, H >> s, W >> s, self.tap_channels[tap], dtype=torch.float32, device=dev)
            _lpips.check(_lpips.lib().mi_lpips_features(C.byref(self.net), dev_ptr(blob, "blob", torch.uint8, 256), blob.numel(), p, n, H, W, int(tap),
                                                        dev_ptr(out), dev_ptr(scratch, "scratch", torch.uint8, 256), scratch.numel(),
                                                        stream_ptr(dev)), "mi_lpips_features")
        return out
