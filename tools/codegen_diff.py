"""Compare the gfx950 code of the kernels in two object directories, kernel by kernel: has a source change reached the generated code?

For every translation unit named (default: every .hip source of every library in build.LIBRARIES), both objects are disassembled the way tools/mfma_hazard_check.py does it (device_asm, kernels_of), and
per kernel the instruction lists are compared, together with the register, scratch and LDS figures of the kernel's metadata note.  Prints
"identical" or the first differing instructions per kernel; exit status 1 if anything differs.

    python -m nerf_pytorch_paeng_amd.build                         # in each of the two trees: fills build_scratch/obj/
    python tools/codegen_diff.py OLD/build_scratch/obj NEW/build_scratch/obj [UNIT.hip ...] [--context N]
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mfma_hazard_check as H  # noqa: E402
from nerf_pytorch_paeng_amd import build  # noqa: E402

UNITS = [src for sources, _, _ in build.LIBRARIES.values() for src in sources if src.endswith(".hip")]
READELF = os.path.join(os.path.dirname(H.OBJDUMP), "llvm-readelf")
FIGURES = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def figures_of(obj: str) -> dict:
    """kernel symbol -> {figure: value} from the code object's amdhsa.kernels metadata."""
    out = {}
    for block in H.device_asm(obj, (READELF, "--notes")).split("\n  - ")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            out[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M) if k in FIGURES}
    return out


def compare(old_dir: str, new_dir: str, context: int = 3, units=UNITS) -> int:
    n_diff = n_same = 0
    for unit in units:
        objs = [os.path.join(d, unit + ".o") for d in (old_dir, new_dir)]
        ins = [H.kernels_of(H.device_asm(o)) for o in objs]
        figs = [figures_of(o) for o in objs]
        for name in sorted(set(ins[0]) | set(ins[1])):
            if name not in figs[0] and name not in figs[1]:
                continue                                        # a label inside a kernel, not a kernel
            if name not in ins[0] or name not in ins[1]:
                print(f"{unit}  {name}: only in the {'new' if name in ins[1] else 'old'} object")
                n_diff += 1
                continue
            a, b = [[body for _, _, body in k[name]] for k in ins]
            fa, fb = figs[0][name], figs[1][name]
            tail = f"{len(a)} instructions, " + ", ".join(f"{k.replace('_count', 's').replace('_fixed_size', '')} {fa[k]}" for k in FIGURES if k in fa)
            if a == b and fa == fb:
                print(f"{unit}  {name}: identical ({tail})")
                n_same += 1
                continue
            n_diff += 1
            print(f"{unit}  {name}: DIFFERS")
            for k in FIGURES:
                if fa.get(k) != fb.get(k):
                    print(f"    {k}: {fa.get(k)} -> {fb.get(k)}")
            if a != b:
                i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
                print(f"    instructions: {len(a)} -> {len(b)}; first difference at instruction {i}:")
                for j in range(max(0, i - context), i + context + 1):
                    x, y = (a[j] if j < len(a) else "-"), (b[j] if j < len(b) else "-")
                    print(f"    {'!' if x != y else ' '} {j:6d}  {x:<64s} | {y}")
                for word in ("v_mfma", "global_load_lds"):
                    print(f"    {word}: {sum(x.startswith(word) for x in a)} -> {sum(y.startswith(word) for y in b)}")
    print(f"{n_diff} of {n_diff + n_same} kernel(s) differ" if n_diff else f"every kernel identical ({n_same} kernels of {len(units)} units)")
    return 1 if n_diff else 0


if __name__ == "__main__":
    argv = sys.argv[1:]
    ctx = int(argv.pop(argv.index("--context") + 1)) if "--context" in argv else 3
    argv = [a for a in argv if a != "--context"]
    sys.exit(compare(argv[0], argv[1], ctx, argv[2:] or UNITS))
