"""sha256 of every weight blob kind and every gather map the host packers produce, over a sweep of synthetic networks.

    python tools/blob_digests.py            rewrite tests/golden/blob_digests.json
    python tools/blob_digests.py --check    recompute and compare (exit status 1 on a difference)

The file pins the packers' output byte for byte (stream order, rounding, header words, side tables): a change to the packing code that is
meant to keep the blobs as they are leaves `git diff tests/golden/blob_digests.json` empty after a regeneration
(tests/test_blob_digests_cpu.py recomputes it).  Host code only: no GPU needed.
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nerf_pytorch_paeng_amd import ops, synthetic      # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "blob_digests.json")
SHAPES = [(2, -1), (8, 4), (8, -1), (16, 4)]            # (D, skip)
ENCODINGS = [(10, 4), (4, 0)]                           # (L_x, L_d)
# kind -> (widths, pack_module keywords, gather map)
KINDS = {
    "fp32": ((64, 128, 256, 384, 512), {}, lambda net: ops.pack_map(net, False)),
    "fp32_bwd": ((128, 256), {"backward": True}, lambda net: ops.pack_map(net, True)),
    "bf16": ((256,), {"bf16": True}, ops.pack_map_bf16),
    "f16s": ((256,), {"f16s": True}, lambda net: ops.pack_map_f16s(net)),
    "f16s_bwd": ((256,), {"f16s": True, "backward": True}, lambda net: ops.pack_map_f16s(net, backward=True)),
}


def _sha(t) -> str:
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def compute() -> dict:
    out = {}
    for W in (64, 128, 256, 384, 512):
        for D, skip in SHAPES:
            for L_x, L_d in ENCODINGS:
                seed = 1000 * D + W + 10 * L_x + (1 if skip < 0 else 0)
                sd = synthetic.make_state_dict(seed, D, W, 3 + 6 * L_x, 3 + 6 * L_d, skips=() if skip < 0 else (skip,))
                net = ops.make_net(D, W, skip, L_x, L_d)
                for kind, (widths, kw, map_fn) in KINDS.items():
                    if W in widths:
                        blob = ops.pack_module(sd, "model_coarse.", net, **kw)
                        out[f"{kind}/D{D}_W{W}_skip{skip}_Lx{L_x}_Ld{L_d}"] = {"seed": seed, "bytes": blob.numel(), "blob": _sha(blob),
                                                                            "map": _sha(map_fn(net))}
    return dict(sorted(out.items()))


def main(argv) -> int:
    got = compute()
    if "--check" in argv:
        want = json.load(open(GOLDEN))
        bad = sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))
        for k in bad:
            print("differs:", k)
        print(f"{len(got)} entries, {len(bad)} differ")
        return 1 if bad else 0
    with open(GOLDEN, "w") as fh:
        json.dump(got, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"wrote {GOLDEN}: {len(got)} entries")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
