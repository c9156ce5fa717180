"""The packers' output is pinned byte for byte, and the 16-bit packers (bf16, split-precision forward and backward: csrc/pack_half.hip)
refuse what they cannot pack -- all on the host: the library loads and the host packers run without a GPU, and every refusal checked
here comes before the first HIP call."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

from nerf_pytorch_paeng_amd import _lib, ops, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1
KINDS = ("bf16", "f16s", "bwd_f16s")


def test_blob_and_map_digests_are_the_committed_ones():
    """tools/blob_digests.py: sha256 of every blob kind and every gather map over a sweep of synthetic networks, against
    tests/golden/blob_digests.json (fp32 forward W = 64 .. 512, fp32 backward W = 128 / 256, the three 16-bit kinds at W = 256; four
    (D, skip) shapes, two encodings).  A difference means the packers write different bytes."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import blob_digests
    want = json.load(open(blob_digests.GOLDEN))
    got = blob_digests.compute()
    assert len(want) == 80 and set(got) == set(want)
    bad = sorted(k for k in want if got[k] != want[k])
    assert not bad, bad


def _fns(kind):
    L = _lib.lib()
    return {"bf16": (L.mi_nerf_packed_bytes_bf16, L.mi_nerf_pack_weights_bf16, L.mi_nerf_pack_map_bf16_len, L.mi_nerf_pack_map_bf16, L.mi_nerf_pack_apply_bf16),
            "f16s": (L.mi_nerf_packed_bytes_f16s, L.mi_nerf_pack_weights_f16s, L.mi_nerf_pack_map_f16s_len, L.mi_nerf_pack_map_f16s, L.mi_nerf_pack_apply_f16s),
            "bwd_f16s": (L.mi_nerf_packed_bytes_bwd_f16s, L.mi_nerf_pack_weights_bwd_f16s, L.mi_nerf_pack_map_bwd_f16s_len, L.mi_nerf_pack_map_bwd_f16s,
                         L.mi_nerf_pack_apply_bwd_f16s)}[kind]


def _apply(kind, net, map_p, flat_p, blob_p, nbytes):
    fn, net_p = _fns(kind)[4], (None if net is None else C.byref(net))
    if kind == "bf16":
        return fn(net_p, map_p, flat_p, blob_p, nbytes, None)
    return fn(net_p, map_p, flat_p, blob_p, nbytes, None, None)


def _error():
    return _lib.lib().mi_nerf_last_error().decode()


def _params(sd, net, prefix="model_coarse."):
    """mi_nerf_params over the arrays of ``sd`` (kept alive by the returned list)."""
    keep = [np.ascontiguousarray(sd[prefix + k], dtype=np.float32) for k in ops.param_names(net)]
    by_name = dict(zip(ops.param_names(net), keep))
    ptr = lambda k: by_name[k].ctypes.data_as(C.c_void_p)
    wx, bx = (C.c_void_p * net.D)(), (C.c_void_p * net.D)()
    for l in range(net.D):
        wx[l], bx[l] = ptr(f"linear_x.{l}.weight"), ptr(f"linear_x.{l}.bias")
    p = _lib.Params(wx, bx, ptr("linear_density.weight"), ptr("linear_density.bias"), ptr("linear_feat.weight"), ptr("linear_feat.bias"),
                    ptr("linear_d.weight"), ptr("linear_d.bias"), ptr("linear_color.weight"), ptr("linear_color.bias"))
    return p, [keep, wx, bx]


@pytest.mark.parametrize("kind", KINDS)
def test_unsupported_networks_are_refused_by_every_entry(kind):
    size_fn, pack_fn, len_fn, map_fn, _ = _fns(kind)
    good = ops.make_net(8, 256, 4)
    n, m = size_fn(C.byref(good)), len_fn(C.byref(good))
    assert n > 1024 and m > 0
    blob, mp = (C.c_char * n)(), (C.c_int32 * m)()
    sd = synthetic.make_state_dict(3, 8, 256)
    p, keep = _params(sd, good)
    assert pack_fn(C.byref(good), C.byref(p), blob, n) == 0 and map_fn(C.byref(good), mp, m) == 0
    variant = "bf16" if kind == "bf16" else "f16-split"
    for D, W, skip, L_x, L_d in ((8, 128, 4, 10, 4), (8, 512, 4, 10, 4), (8, 64, 4, 10, 4),                 # these kinds exist for W = 256 only
                                 (1, 256, -1, 10, 4), (17, 256, 4, 10, 4), (8, 256, 4, 11, 4), (8, 256, 4, 10, 5), (8, 256, -2, 10, 4),
                                 (8, 256, 4, -1, 4), (8, 256, 4, 10, -1)):
        bad = ops.make_net(D, W, skip, L_x, L_d)
        assert size_fn(C.byref(bad)) == 0 and _error(), (D, W, skip, L_x, L_d)
        assert len_fn(C.byref(bad)) == 0
        assert pack_fn(C.byref(bad), C.byref(p), blob, n) == EINVAL
        assert map_fn(C.byref(bad), mp, m) == EINVAL
        assert _apply(kind, bad, mp, blob, blob, n) == EINVAL and "HIP error" not in _error()
        if W != 256:
            assert variant in _error() and "W=256" in _error(), _error()
    assert size_fn(None) == 0 and len_fn(None) == 0
    assert pack_fn(None, C.byref(p), blob, n) == EINVAL and map_fn(None, mp, m) == EINVAL and _apply(kind, None, mp, blob, blob, n) == EINVAL


@pytest.mark.parametrize("kind", KINDS)
def test_short_and_misaligned_buffers_are_refused(kind):
    size_fn, pack_fn, len_fn, map_fn, _ = _fns(kind)
    net = ops.make_net(2, 256, -1, 4, 0)
    n, m = size_fn(C.byref(net)), len_fn(C.byref(net))
    sd = synthetic.make_state_dict(3, 2, 256, 27, 3, skips=())
    p, keep = _params(sd, net)
    blob, mp = (C.c_char * (n + 32))(), (C.c_int32 * m)()
    assert pack_fn(C.byref(net), C.byref(p), blob, n - 1) == EINVAL and "too small" in _error()
    assert pack_fn(C.byref(net), C.byref(p), blob, 0) == EINVAL
    assert pack_fn(C.byref(net), None, blob, n) == EINVAL and pack_fn(C.byref(net), C.byref(p), None, n) == EINVAL
    assert map_fn(C.byref(net), mp, m - 1) == EINVAL and "too small" in _error()
    assert map_fn(C.byref(net), mp, 0) == EINVAL and map_fn(C.byref(net), None, m) == EINVAL
    # the device-side packer: host addresses stand in for the device pointers -- every refusal comes before a launch
    base = C.addressof(blob)
    aligned = (base + 15) & ~15
    for map_p, flat_p, blob_p, nbytes in ((mp, blob, aligned, n - 1), (mp, blob, aligned + 4, n), (mp, blob, aligned + 8, n), (None, blob, aligned, n),
                                          (mp, None, aligned, n), (mp, blob, None, n)):
        assert _apply(kind, net, map_p, flat_p, blob_p, nbytes) == EINVAL and "HIP error" not in _error(), (map_p, flat_p, blob_p, nbytes)
    assert _apply(kind, net, mp, blob, aligned + 4, n) == EINVAL and "16-byte aligned" in _error()


@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("value", [float("nan"), 65504.0, -65504.0, 1.0e6, float("inf")])
def test_split_precision_host_packers_refuse_weights_beyond_f16(value, backward):
    """|w| < 65504 and not NaN, or the host packers refuse the network (the forward one names the parameter); the bf16 packer takes it."""
    size_fn, pack_fn = _fns("bwd_f16s" if backward else "f16s")[:2]
    net = ops.make_net(3, 256, 0)
    sd = {k: np.array(v) for k, v in synthetic.make_state_dict(3, 3, 256, skips=(0,)).items()}
    n = size_fn(C.byref(net))
    blob = (C.c_char * n)()
    sd["model_coarse.linear_feat.weight"][200, 17] = 65503.0                  # the largest magnitudes that fit
    sd["model_coarse.linear_x.2.weight"][5, 100] = -65503.0
    p, keep = _params(sd, net)
    assert pack_fn(C.byref(net), C.byref(p), blob, n) == 0
    for key in ("linear_feat.weight", "linear_x.1.weight", "linear_d.weight"):
        bad = dict(sd)
        bad["model_coarse." + key] = np.array(sd["model_coarse." + key])
        bad["model_coarse." + key][7, 70] = value                            # column 70: an activation column of the skip layer and of linear_d
        p, keep = _params(bad, net)
        assert pack_fn(C.byref(net), C.byref(p), blob, n) == EINVAL, (key, value)
        assert "f16-split" in _error() and "HIP error" not in _error()
        if not backward:
            where = f"{key.replace('.1.', '.')}[{7 * bad['model_coarse.' + key].shape[1] + 70}]"      # the tensor (trunk layers share a name) and the element
            assert where in _error(), (where, _error())
        n16 = _lib.lib().mi_nerf_packed_bytes_bf16(C.byref(net))
        assert _lib.lib().mi_nerf_pack_weights_bf16(C.byref(net), C.byref(p), (C.c_char * n16)(), n16) == 0
