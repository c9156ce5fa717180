"""libmi_nerf_scene.so / include/mi_nerf_scene.h without a GPU: the header is C99 on its own and a C program links against the library; the
header, the ctypes table (nerf_pytorch_paeng_amd/_scene.py) and the library's dynamic symbols name the same entries; the library exports
nothing of the other three and libmi_nerf.so is what it was (exactly the names of _lib.SIGNATURES); every refusal answers MI_SCENE_EINVAL with
a message before any HIP call.  ``field_rule`` (numpy fp32, written from the header, not from the kernel) is the restatement the GPU tests
compare mi_scene_field_rays with; it checks itself on hand-made points."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1
f32 = np.float32
SPHERE, BOX, CYLINDER = 0, 1, 2


# ---------------------------------------------------------------------------------------------------
# restatement (from include/mi_nerf_scene.h)
# ---------------------------------------------------------------------------------------------------
def P(kind, c, h, sigma=64.0, rgb_raw=((1.0, 2.0, 3.0), (-1.0, -2.0, -3.0)), freq=0.0, axis=0):
    """A primitive as plain data: the fields of mi_scene_prim."""
    h = tuple(h) + (0.0,) * (3 - len(tuple(h)))
    return dict(kind=kind, axis=axis, c=tuple(c), h=h, sigma=sigma, rgb_raw=tuple(tuple(r) for r in rgb_raw), freq=freq)


def field_rule(prims, rays, z):
    """THE FIELD RULE: prims (dicts of ``P``), rays [n,6], z [n,S] -> raw [n,S,4] fp32.  Every operation is one fp32 numpy operation."""
    rays, z = np.asarray(rays, f32), np.asarray(z, f32)
    raw = np.zeros(z.shape + (4,), f32)
    with np.errstate(invalid="ignore", over="ignore"):
        p = [(rays[:, i:i + 1] + (rays[:, 3 + i:4 + i] * z).astype(f32)).astype(f32) for i in range(3)]
        for pr in reversed(prims):                                  # an earlier primitive overwrites a later one: the first in list order wins
            q = [(p[i] - f32(pr["c"][i])).astype(f32) for i in range(3)]
            h = [f32(v) for v in pr["h"]]
            if pr["kind"] == SPHERE:
                inside = (((q[0] * q[0]).astype(f32) + (q[1] * q[1]).astype(f32)).astype(f32) + (q[2] * q[2]).astype(f32)).astype(f32) <= f32(h[0] * h[0])
            elif pr["kind"] == BOX:
                inside = (np.abs(q[0]) <= h[0]) & (np.abs(q[1]) <= h[1]) & (np.abs(q[2]) <= h[2])
            else:
                a = pr["axis"]
                b, c = [i for i in range(3) if i != a]
                inside = (np.abs(q[a]) <= h[1]) & (((q[b] * q[b]).astype(f32) + (q[c] * q[c]).astype(f32)).astype(f32) <= f32(h[0] * h[0]))
            colour = np.zeros(z.shape, np.int32)
            if pr["freq"] > 0:
                k = [np.floor((q[i] * f32(pr["freq"])).astype(f32)) for i in range(3)]
                k = [np.where(np.isfinite(ki), ki, 0).astype(np.int32) for ki in k]
                colour = (k[0] + k[1] + k[2]) & 1
            val = np.asarray(pr["rgb_raw"], f32)[colour]            # [n,S,3]
            raw[..., :3] = np.where(inside[..., None], val, raw[..., :3])
            raw[..., 3] = np.where(inside, f32(pr["sigma"]), raw[..., 3])
    return raw


def c_prims(scene_mod, prims):
    """The ctypes array of plain-data primitives."""
    arr = (scene_mod.Prim * len(prims))()
    for i, pr in enumerate(prims):
        arr[i] = scene_mod.Prim(pr["kind"], pr["axis"], (C.c_float * 3)(*pr["c"]), (C.c_float * 3)(*pr["h"]), pr["sigma"],
                                ((C.c_float * 3) * 2)((C.c_float * 3)(*pr["rgb_raw"][0]), (C.c_float * 3)(*pr["rgb_raw"][1])), pr["freq"])
    return arr


def plain_prims(scene):
    """A scenes.SolidScene as the plain data ``field_rule`` takes."""
    return [P(p.kind, tuple(p.c), tuple(p.h), p.sigma, (tuple(p.rgb_raw[0]), tuple(p.rgb_raw[1])), p.freq, p.axis) for p in scene.prims]


# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scn():
    """The library is built when the tree is fresh (a no-op when it is up to date), like tests/conftest.py does for libmi_nerf.so."""
    from nerf_pytorch_paeng_amd import _scene
    from nerf_pytorch_paeng_amd.build import build_scene_library
    build_scene_library()
    _scene.lib()
    return _scene


def _along_x(xs, y=0.0, zc=0.0):
    """One ray from the origin offset (0, y, zc) along +x: depth == x coordinate."""
    return np.array([[0.0, y, zc, 1.0, 0.0, 0.0]], f32), np.array([xs], f32)


def test_field_rule_restatement_on_hand_made_points():
    A, B = ((1.0, 2.0, 3.0), (-1.0, -2.0, -3.0)), ((5.0, 6.0, 7.0), (-5.0, -6.0, -7.0))
    # a box whose face lies exactly on a representable number: q == h is inside, the next float up is outside
    box = P(BOX, (1.0, 0.0, 0.0), (0.5, 0.25, 0.25), sigma=8.0, rgb_raw=A)
    up = float(np.nextafter(f32(1.5), f32(2.0)))
    rays, z = _along_x([0.4, 0.5, 1.0, 1.5, up, float("nan")])
    got = field_rule([box], rays, z)[0]
    assert got[:, 3].tolist() == [0.0, 8.0, 8.0, 8.0, 0.0, 0.0]
    assert got[1, :3].tolist() == [1.0, 2.0, 3.0] and got[0].tolist() == [0.0] * 4 and got[5].tolist() == [0.0] * 4       # a NaN is outside
    rays, z = _along_x([1.0, 1.0], y=0.25)
    assert field_rule([box], rays, z)[0, 0, 3] == 8.0                                        # on the y face
    rays, z = _along_x([1.0], y=float(np.nextafter(f32(0.25), f32(1.0))))
    assert field_rule([box], rays, z)[0, 0, 3] == 0.0
    # a sphere: the surface point (r, 0, 0) is inside
    sph = P(SPHERE, (0.0, 0.0, 0.0), (0.5,), sigma=4.0, rgb_raw=B)
    rays, z = _along_x([-0.5, 0.0, 0.5, float(np.nextafter(f32(0.5), f32(1.0)))])
    assert field_rule([sph], rays, z)[0, :, 3].tolist() == [4.0, 4.0, 4.0, 0.0]
    # a cylinder along y: half-height on y, radius over (x, z)
    cyl = P(CYLINDER, (0.0, 0.0, 0.0), (0.5, 2.0), sigma=2.0, axis=1)
    rays, z = _along_x([0.5, 0.51], y=2.0)
    assert field_rule([cyl], rays, z)[0, :, 3].tolist() == [2.0, 0.0]
    rays, z = _along_x([0.0], y=2.5)
    assert field_rule([cyl], rays, z)[0, 0, 3] == 0.0
    cylx = dict(cyl, axis=0)                                                                 # along x: x is the height now
    rays, z = _along_x([1.9, 2.0, 2.1], y=0.3, zc=0.4)                                       # 0.09 + 0.16 = 0.25 <= 0.25 in fp32
    assert field_rule([cylx], rays, z)[0, :, 3].tolist() == [2.0, 2.0, 0.0]
    # two overlapping primitives: list order wins, whichever way round
    rays, z = _along_x([0.25, 0.6, 1.4])
    assert field_rule([sph, box], rays, z)[0, :, 3].tolist() == [4.0, 8.0, 8.0]
    assert field_rule([box, sph], rays, z)[0, :, 3].tolist() == [4.0, 8.0, 8.0]             # 0.25 is in the sphere alone
    rays, z = _along_x([0.5])
    assert field_rule([sph, box], rays, z)[0, 0].tolist() == [5.0, 6.0, 7.0, 4.0] and field_rule([box, sph], rays, z)[0, 0].tolist() == [1.0, 2.0, 3.0, 8.0]
    # the checker in the primitive's frame, parity at negative q: floor(-0.5) = -1, and -1 & 1 = 1
    chk = P(BOX, (0.0, 0.0, 0.0), (2.0, 2.0, 2.0), rgb_raw=A, freq=1.0)
    rays, z = _along_x([-1.5, -0.5, 0.5, 1.5], y=0.5, zc=0.5)                                # k = (-2, -1, 0, 1) + 0 + 0
    assert field_rule([chk], rays, z)[0, :, 0].tolist() == [1.0, -1.0, 1.0, -1.0]
    rays, z = _along_x([-0.5, 0.5], y=-0.5, zc=0.5)                                          # k = (-1, 0) - 1 + 0
    assert field_rule([chk], rays, z)[0, :, 0].tolist() == [1.0, -1.0]
    rays, z = _along_x([-0.5], y=-0.5, zc=-0.5)                                              # -3: odd
    assert field_rule([chk], rays, z)[0, :, 0].tolist() == [-1.0]


def test_header_compiles_as_c99_and_the_library_links_and_answers(tmp_path, scn):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not found")
    pkg = os.path.dirname(scn.LIB_PATH)
    exe = str(tmp_path / "scene_consumer")
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "c_abi", "scene_consumer.c"), "-L", pkg, "-lmi_nerf_scene", f"-Wl,-rpath,{pkg}", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"scene c_abi consumer ok: ABI {scn.ABI_VERSION}" in run.stdout


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if " T " in ln}


def test_header_table_and_symbols_agree_and_the_libraries_do_not_mix(scn):
    from nerf_pytorch_paeng_amd import _lib
    from nerf_pytorch_paeng_amd.build import build_library
    build_library()
    hdr = open(os.path.join(ROOT, "include", "mi_nerf_scene.h")).read()
    declared = set(re.findall(r"\b(mi_scene_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(scn.SIGNATURES), declared ^ set(scn.SIGNATURES)
    new = _exports(scn.LIB_PATH)
    assert {n for n in new if n.startswith("mi_scene_")} == declared
    assert not [n for n in new if n.startswith("mi_nerf_") or n.startswith("mi_occ_") or n.startswith("mi_iqa_")]
    old = _exports(_lib.LIB_PATH)
    assert {n for n in old if n.startswith("mi_")} == set(_lib.SIGNATURES) and len(_lib.SIGNATURES) == 68       # libmi_nerf.so: its entries and nothing of this
    assert not set(scn.SIGNATURES) & set(_lib.SIGNATURES)
    for other in ("mi_nerf.h", "mi_nerf_occ.h", "mi_nerf_iqa.h"):
        assert "mi_scene_" not in open(os.path.join(ROOT, "include", other)).read()
    assert '#include "mi_nerf' not in hdr                                                   # the header stands alone
    assert scn.lib().mi_scene_abi_version() == scn.ABI_VERSION == int(re.search(r"#define MI_SCENE_ABI_VERSION (\d+)", hdr).group(1))
    assert (scn.MAX_PRIMS, scn.MAX_SAMPLES) == tuple(int(re.search(rf"#define {n} (\d+)", hdr).group(1)) for n in ("MI_SCENE_MAX_PRIMS", "MI_SCENE_MAX_SAMPLES"))
    assert C.sizeof(scn.Prim) == 64
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert [n for n in sorted(declared) if n not in doc] == []


def test_the_library_stands_alone(scn):
    dyn = subprocess.run(["readelf", "-d", scn.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libmi_nerf" not in dyn
    und = subprocess.run(["nm", "-D", "--undefined-only", scn.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not [ln for ln in und.splitlines() if ln.split()[-1].startswith("mi_")]


# ---------------------------------------------------------------------------------------------------
GOOD = P(BOX, (0.0, 0.0, 0.0), (0.5, 0.5, 0.5))
NAN, INF = float("nan"), float("inf")
PRIM_REFUSALS = {
    "kind -1": dict(kind=-1),
    "kind 3": dict(kind=3),
    "axis -1": dict(kind=CYLINDER, axis=-1),
    "axis 3": dict(kind=CYLINDER, axis=3),
    "centre NaN": dict(c=(0.0, NAN, 0.0)),
    "centre inf": dict(c=(INF, 0.0, 0.0)),
    "box extent zero": dict(h=(0.5, 0.0, 0.5)),
    "box extent negative": dict(h=(0.5, 0.5, -0.5)),
    "box extent NaN": dict(h=(NAN, 0.5, 0.5)),
    "box extent inf": dict(h=(0.5, INF, 0.5)),
    "sphere radius zero": dict(kind=SPHERE, h=(0.0, 0.5, 0.5)),
    "sphere radius inf": dict(kind=SPHERE, h=(INF, 0.5, 0.5)),
    "sphere radius squared overflows": dict(kind=SPHERE, h=(1e20, 0.5, 0.5)),
    "cylinder radius negative": dict(kind=CYLINDER, h=(-0.5, 0.5, 0.5)),
    "cylinder half-height zero": dict(kind=CYLINDER, h=(0.5, 0.0, 0.5)),
    "cylinder half-height NaN": dict(kind=CYLINDER, h=(0.5, NAN, 0.5)),
    "sigma zero": dict(sigma=0.0),
    "sigma negative": dict(sigma=-1.0),
    "sigma NaN": dict(sigma=NAN),
    "sigma inf": dict(sigma=INF),
    "colour NaN": dict(rgb_raw=((0.0, NAN, 0.0), (0.0, 0.0, 0.0))),
    "second colour inf": dict(rgb_raw=((0.0, 0.0, 0.0), (0.0, 0.0, INF))),
    "freq negative": dict(freq=-1.0),
    "freq NaN": dict(freq=NAN),
}


@pytest.mark.parametrize("case", sorted(PRIM_REFUSALS))
def test_a_bad_primitive_is_refused_by_every_entry_before_any_hip_call(scn, case):
    """The pointers are made-up addresses that are never dereferenced: every call here is refused before the first HIP call (a call that got
    as far as one would answer MI_SCENE_EHIP, "HIP error ... no ROCm-capable device", on a machine without a GPU)."""
    L = scn.lib()
    arr = c_prims(scn, [GOOD, dict(GOOD, **PRIM_REFUSALS[case])])
    for rc in (L.mi_scene_check(arr, 2), L.mi_scene_field_rays(arr, 2, 0x1000, 0x2000, 4, 8, 0x3000, None),
               L.mi_scene_render(arr, 2, 0x1000, 4, 2.0, 6.0, 64, 0x2000, 0x3000, 0x4000, 0x5000, None)):
        msg = scn.last_error()
        assert rc == EINVAL, (case, rc, msg)
        assert msg and "prim 1" in msg and "HIP error" not in msg, (case, msg)
    assert L.mi_scene_check(arr, 1) == 0                            # the good one alone passes


def test_unused_extents_are_not_read(scn):
    arr = c_prims(scn, [P(SPHERE, (0, 0, 0), (0.5, NAN, -1.0)), P(CYLINDER, (0, 0, 0), (0.5, 0.5, NAN), axis=1)])
    assert scn.lib().mi_scene_check(arr, 2) == 0, scn.last_error()


GOOD_RENDER = dict(prims=True, n_prims=1, rays=0x1000, n=256, near=2.0, far=6.0, S=64, rgb=0x2000)
RENDER_REFUSALS = {
    "NULL prims": dict(prims=False),
    "n_prims 0": dict(n_prims=0),
    "n_prims 17": dict(n_prims=17),
    "NULL rays": dict(rays=None),
    "NULL rgb": dict(rgb=None),
    "negative n": dict(n=-1),
    "S 0": dict(S=0),
    "S 4097": dict(S=4097),
    "far == near": dict(far=2.0),
    "far < near": dict(far=1.0),
    "near NaN": dict(near=NAN),
    "far inf": dict(far=INF),
}


@pytest.mark.parametrize("case", sorted(RENDER_REFUSALS))
def test_render_refusals_answer_einval_with_a_message_before_any_hip_call(scn, case):
    a = dict(GOOD_RENDER, **RENDER_REFUSALS[case])
    arr = c_prims(scn, [GOOD] * 17)
    L = scn.lib()
    rc = L.mi_scene_render(arr if a["prims"] else None, a["n_prims"], a["rays"], a["n"], a["near"], a["far"], a["S"], a["rgb"], None, None, None, None)
    msg = scn.last_error()
    assert rc == EINVAL, (case, rc, msg)
    assert msg and "HIP error" not in msg, (case, msg)


GOOD_FIELD = dict(prims=True, n_prims=1, rays=0x1000, z=0x2000, n=256, S=64, raw=0x3000)
FIELD_REFUSALS = {
    "NULL prims": dict(prims=False),
    "n_prims 0": dict(n_prims=0),
    "n_prims 17": dict(n_prims=17),
    "NULL rays": dict(rays=None),
    "NULL z": dict(z=None),
    "NULL raw": dict(raw=None),
    "unaligned raw": dict(raw=0x3004),
    "negative n": dict(n=-1),
    "S 0": dict(S=0),
    "too many samples for one launch": dict(n=1 << 33),
}


@pytest.mark.parametrize("case", sorted(FIELD_REFUSALS))
def test_field_refusals_answer_einval_with_a_message_before_any_hip_call(scn, case):
    a = dict(GOOD_FIELD, **FIELD_REFUSALS[case])
    arr = c_prims(scn, [GOOD] * 17)
    L = scn.lib()
    rc = L.mi_scene_field_rays(arr if a["prims"] else None, a["n_prims"], a["rays"], a["z"], a["n"], a["S"], a["raw"], None)
    msg = scn.last_error()
    assert rc == EINVAL, (case, rc, msg)
    assert msg and "HIP error" not in msg, (case, msg)


def test_zero_rays_are_accepted_without_a_launch(scn):
    arr = c_prims(scn, [GOOD])
    L = scn.lib()
    assert L.mi_scene_render(arr, 1, 0x1000, 0, 2.0, 6.0, 64, 0x2000, None, None, None, None) == 0, scn.last_error()
    assert L.mi_scene_field_rays(arr, 1, 0x1000, 0x2000, 0, 64, 0x3000, None) == 0, scn.last_error()
    assert L.mi_scene_render(arr, 1, None, 0, 2.0, 6.0, 64, None, None, None, None, None) == 0, scn.last_error()     # empty buffers have NULL pointers
    assert L.mi_scene_field_rays(arr, 1, None, None, 0, 64, None, None) == 0, scn.last_error()
    assert L.mi_scene_render(arr, 1, None, 0, 2.0, 6.0, 0, None, None, None, None, None) == EINVAL                     # the other arguments are still checked
    assert L.mi_scene_check(None, 1) == EINVAL and "NULL" in scn.last_error()


def test_python_surface_without_a_gpu(scn):
    from nerf_pytorch_paeng_amd import scenes
    from nerf_pytorch_paeng_amd._lib import MiNerfError
    s = scenes.sphere((0.1, 0.2, 0.3), 0.5, (0.25, 0.5, 0.75))
    assert (s.kind, tuple(s.c), s.h[0], s.freq) == (SPHERE, (f32(0.1), f32(0.2), f32(0.3)), 0.5, 0.0)
    want = [float(f32(math.log(c / (1.0 - c)))) for c in (0.25, 0.5, 0.75)]                  # float64 logit, rounded to fp32 once
    assert list(s.rgb_raw[0]) == want and list(s.rgb_raw[1]) == want
    b = scenes.box((0, 0, 0), (0.1, 0.2, 0.3), (0.2, 0.2, 0.2), rgb2=(0.9, 0.9, 0.9), freq=4.0, sigma=64.0)
    assert (b.kind, tuple(b.h), b.freq, b.sigma) == (BOX, (f32(0.1), f32(0.2), f32(0.3)), 4.0, 64.0) and list(b.rgb_raw[0]) != list(b.rgb_raw[1])
    c = scenes.cylinder((0, 0, 0), 0.2, 0.4, (0.5, 0.5, 0.5), axis=1)
    assert (c.kind, c.axis, c.h[0], c.h[1]) == (CYLINDER, 1, f32(0.2), f32(0.4))
    scene = scenes.SolidScene([s, b, c])
    assert len(scene) == 3
    for bad in ((0.0, 0.5, 0.5), (0.5, 1.0, 0.5), (0.5, 0.5), (0.5, -0.1, 0.5)):
        with pytest.raises(MiNerfError, match="colour"):
            scenes.sphere((0, 0, 0), 0.5, bad)
    with pytest.raises(MiNerfError, match="second colour"):
        scenes.box((0, 0, 0), (0.1, 0.1, 0.1), (0.5, 0.5, 0.5), freq=2.0)
    with pytest.raises(MiNerfError):
        scenes.SolidScene([])
    with pytest.raises(MiNerfError):
        scenes.SolidScene([s] * 17)
    for bad in (scenes.sphere((0, 0, 0), -0.5, (0.5, 0.5, 0.5)), scenes.cylinder((0, 0, 0), 0.2, 0.4, (0.5, 0.5, 0.5), axis=3),
                scenes.box((0, 0, 0), (0.1, 0.0, 0.1), (0.5, 0.5, 0.5)), scenes.sphere((0, 0, 0), 0.5, (0.5, 0.5, 0.5), sigma=0.0)):
        with pytest.raises(MiNerfError, match="mi_scene_check"):
            scenes.SolidScene([bad])
    # the default scene: inside the box +-1.2 (so inside near / far = 2 / 6 from radius 4), one checkered box, a sphere and a cylinder
    d = scenes.SolidScene.default()
    kinds = [p.kind for p in d.prims]
    assert SPHERE in kinds and CYLINDER in kinds and kinds.count(BOX) >= 3 and sum(1 for p in d.prims if p.kind == BOX and p.freq > 0) == 1
    for p in d.prims:
        ext = {SPHERE: (p.h[0],) * 3, BOX: tuple(p.h)}.get(p.kind)
        if ext is None:
            ext = tuple(p.h[1] if i == p.axis else p.h[0] for i in range(3))
        assert all(abs(p.c[i]) + ext[i] <= 1.2 for i in range(3))
        assert p.sigma * (4.0 / 1024) >= 16.0                                               # one sample of the default render is opaque
    # no GPU: the device entries refuse host tensors loudly, they do not fall back
    with pytest.raises(MiNerfError, match="HIP device"):
        d.render(torch.zeros(4, 6), 2.0, 6.0)
    with pytest.raises(MiNerfError, match="HIP device"):
        d.field(torch.zeros(4, 6), torch.zeros(4, 8))
    with pytest.raises(MiNerfError):
        d.field(torch.zeros(4, 6), torch.zeros(5, 8))
    K = scenes.scaled_camera((32, 48))
    assert K.shape == (3, 3) and K[0][2] == 24 and K[1][2] == 16
