"""The launch plan of the persistent MLP kernels (csrc/walk_plan.h) is integer arithmetic in a header without device code: a host program
(tests/c_abi/walk_plan_enum.cpp) enumerates, for every wave and iteration, the unit that walk_unit returns, and the fp32 kernels'
incremental (ray, chunk) form of the same walk.  Checked here: every unit is dealt exactly once, a ray-major wave stays on one ray for a
ray's worth of units, and the decision and iteration count are the launchers' formulas, restated below."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID, WAVES = 2, 4
SMALL = [(n_rays, upr, GRID, WAVES) for n_rays in (1, 3, 7, 8, 9, 17) for upr in (1, 2, 3, 6)]
NAMED = (1500, 6, 256, 4)          # the kernel comment's case: 1500 rays x 6 tiles on 1024 waves, 12 ray-major steps against 9 flat ones


def _ceil(a, b):
    return -(-a // b)


def _plan(n_rays, upr, grid, waves):
    """ray_major, n_iter as the launchers computed them before the plan had a header of its own: workgroups of `waves` units dealt to
    `grid` workgroups round by round, whole rays only when every wave gets one and it costs no round more."""
    nw = grid * waves
    n_wg = _ceil(n_rays * upr, waves)
    it_flat = _ceil(n_wg, grid)
    it_ray = _ceil(n_rays, nw) * upr
    ray_major = n_rays >= nw and it_ray <= it_flat
    return ray_major, (it_ray if ray_major else it_flat)


@pytest.fixture(scope="module")
def walks(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("walk_plan") / "walk_plan_enum")
    r = subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "nerf_pytorch_paeng_amd", "csrc"),
                        os.path.join(ROOT, "tests", "c_abi", "walk_plan_enum.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cases = SMALL + [NAMED]
    run = subprocess.run([exe] + [str(v) for c in cases for v in c], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    out, cur = {}, None
    for line in run.stdout.splitlines():
        tag, *vals = line.split()
        vals = [int(v) for v in vals]
        if tag == "P":
            cur = {"ray_major": bool(vals[0]), "n_iter": vals[1], "U": {}, "T": {}}
            out[cases[len(out)]] = cur
        else:
            cur[tag][vals[0]] = vals[1:]
    assert len(out) == len(cases)
    return out


@pytest.mark.parametrize("case", SMALL + [NAMED], ids=lambda c: "x".join(str(v) for v in c))
def test_walk_deals_every_unit_once_and_matches_the_launchers_formulas(walks, case):
    n_rays, upr, grid, waves = case
    w = walks[case]
    nw, n_units = grid * waves, n_rays * upr
    assert (w["ray_major"], w["n_iter"]) == _plan(n_rays, upr, grid, waves)
    assert sorted(w["U"]) == list(range(nw)) and all(len(u) == w["n_iter"] for u in w["U"].values())
    dealt = sorted(u for units in w["U"].values() for u in units if u < n_units)
    assert dealt == list(range(n_units))                       # every unit exactly once
    if w["ray_major"]:
        for units in w["U"].values():                          # a wave's consecutive upr units: one ray, first unit to last
            for i in range(0, len(units), upr):
                assert units[i:i + upr] == list(range(units[i], units[i] + upr)) and units[i] % upr == 0
    assert w["T"] == w["U"]                                    # stepping (ray, chunk) visits the closed form's tiles


def test_the_named_case_walks_flat(walks):
    w = walks[NAMED]
    assert _ceil(1500, 1024) * 6 == 12 and not w["ray_major"] and w["n_iter"] == 9


def test_both_branches_are_among_the_small_cases(walks):
    kinds = {walks[c]["ray_major"] for c in SMALL}
    assert kinds == {True, False}
