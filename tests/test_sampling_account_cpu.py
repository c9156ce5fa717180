"""The sample-accounting check of tests/sampling_account.py, on the CPU: the oracle and the reference-generated fixtures leave ZERO
samples unaccounted on every weight family and shape (so a GPU test may ask the same of the kernels), and every planted bug --
among them one that the flip counts of the GPU tests cannot see -- is reported."""
import time

import numpy as np
import pytest
import torch

from oracle import restate as R
from tests import sampling_account as SA

T = torch.from_numpy
N_ROWS = 256


def _bins(n, B, seed, rng):
    return SA.sorted_depths(n, B, seed, rng[0], rng[1], tie=True)


@pytest.mark.parametrize("rng", [(2.0, 6.0), (0.0, 1.0)])
@pytest.mark.parametrize("N", [1, 6, 128])
@pytest.mark.parametrize("B", [2, 3, 63, 191, 1023])
def test_oracle_leaves_no_sample_unaccounted(B, N, rng):
    """oracle.restate.sample_pdf (fp32, the reference's arithmetic) on every family: deterministic u (holds 0 and exactly 1) and random u
    holding 0 and nextafter(1, 0); one tied pair of bins per row; depth ranges of the blender scenes and of NDC."""
    seed = B * 7 + N
    bins = _bins(N_ROWS, B, seed, rng)
    worst = 0.0
    for name, fam in SA.FAMILIES.items():
        w = fam(N_ROWS, B, seed + 1)
        for det in (True, False):
            u = SA.det_uniforms(N) if det else SA.edge_uniforms(N_ROWS, N, seed + 2)
            s = R.sample_pdf(bins, w, N, det, None if det else u)
            acc = SA.account(bins, w, u, s)
            steep = acc.residual[acc.flat == 0]
            worst = max(worst, float(steep.max()) if steep.numel() else 0.0)
            assert int(acc.bad.sum()) == 0, (name, det, acc.worst())
    print(f"B={B} N={N} range={rng}: largest steep-bin residual {worst:.2e} = {worst / SA.delta_u(B):.2f} delta_u")


def test_golden_F4_samples_are_accounted_for(golden):
    g = golden("F4_sample_pdf")
    bins, w, u = T(g["bins"]), T(g["weights"]), T(g["u"])
    for key, uu in (("samples_rand", u), ("samples_det", SA.det_uniforms(128))):
        acc = SA.account(bins, w, uu, T(g[key]))
        print(f"F4 {key}: {acc.worst()}")
        assert int(acc.bad.sum()) == 0, key
    acc = SA.account(torch.linspace(2, 6, 5)[None], torch.tensor([[0.1, 0.0, 0.6, 0.3]]), SA.det_uniforms(6), T(g["kat_samples"]))
    assert int(acc.bad.sum()) == 0, acc.worst()


@pytest.mark.parametrize("tag", ["legoA", "legoA_det", "plumbP", "fernN"])
def test_golden_F8_fine_depths_are_accounted_for(golden, tag):
    """The reference's own fine depths: the oracle's new samples merge, sorted, into exactly the fixture's z_f; none is unaccounted."""
    g = golden("F8_render_rays")
    Nf = int(g[f"{tag}_Nf"])
    if Nf == 0:
        assert f"{tag}_z_f" not in g          # a coarse-only case: nothing was resampled
        return
    det = float(g[f"{tag}_perturb"]) == 0.0
    z_c, w_c = T(g[f"{tag}_z_c"]), T(g[f"{tag}_weights_c"])
    u = None if det else T(g[f"{tag}_u"])
    z_f, z_new = R.fine_z(z_c, w_c, Nf, det, u)
    assert torch.equal(z_f, T(g[f"{tag}_z_f"]))
    acc = SA.fine_account(z_c, w_c, u, z_new)
    print(f"F8 {tag}: {acc.worst()}")
    assert int(acc.bad.sum()) == 0


# ------------------------------------------------------------------------------------------------------------------------
# planted bugs: an fp32 copy of oracle.restate.sample_pdf with one thing wrong
# ------------------------------------------------------------------------------------------------------------------------
def _buggy_sample_pdf(bins, weights, u, bug):
    w = weights if bug == "no_floor" else weights + 1e-5
    total = torch.sum(w[..., :-1] if bug == "total_without_last" else w, -1, keepdim=True)
    cdf = torch.cumsum(w / total, -1)
    cdf = torch.cat([torch.zeros_like(cdf[..., :1]), cdf], -1)
    u = u.to(torch.float32).expand(bins.shape[0], u.shape[-1]).contiguous()
    idx = torch.searchsorted(cdf, u, right=True)
    if bug == "one_in_300_up_a_bin":
        pick = torch.zeros(idx.numel(), dtype=torch.bool)
        pick[::300] = True
        idx = idx + pick.view_as(idx).long()
    lo = (idx - 1).clamp(min=0, max=cdf.shape[-1] - 1)
    hi = (idx + 1 if bug == "above_one_bin_too_far" else idx).clamp(max=cdf.shape[-1] - 1)
    cdf_lo, cdf_hi = torch.gather(cdf, -1, lo), torch.gather(cdf, -1, hi)
    bin_lo, bin_hi = torch.gather(bins, -1, lo), torch.gather(bins, -1, hi)
    denom = cdf_hi - cdf_lo
    if bug != "no_denom_branch":
        denom = torch.where(denom < 1e-5, torch.ones_like(denom), denom)
    s = bin_lo + (u - cdf_lo) / denom * (bin_hi - bin_lo)
    if bug == "one_nan":
        s[3, 5] = float("nan")
    if bug == "one_outside_the_hull":
        s[3, 5] = bins[3, -1] + (bins[3, -1] - bins[3, -2])
    return s


BUGS = ["no_floor", "above_one_bin_too_far", "total_without_last", "one_in_300_up_a_bin", "no_denom_branch", "one_nan", "one_outside_the_hull"]


def _case(family, B=63, N=128, n=N_ROWS, seed=5):
    bins = SA.sorted_depths(n, B, seed, tie=False)
    return bins, SA.FAMILIES[family](n, B, seed + 1), SA.edge_uniforms(n, N, seed + 2)


@pytest.mark.parametrize("bug", BUGS)
def test_planted_bug_is_reported(bug):
    shares = {}
    for family in SA.FAMILIES:
        bins, w, u = _case(family)
        assert int(SA.unaccounted(bins, w, u, _buggy_sample_pdf(bins, w, u, None)).sum()) == 0, family      # the copy itself is right
        shares[family] = float(SA.unaccounted(bins, w, u, _buggy_sample_pdf(bins, w, u, bug)).float().mean())
    print(f"{bug}: share of samples unaccounted per family {({k: round(v, 4) for k, v in shares.items()})}")
    assert max(shares.values()) > 0.0, shares
    if bug in ("no_floor", "above_one_bin_too_far", "total_without_last"):
        assert max(shares.values()) > 0.5, shares                # a gross error is seen on most samples of some family, not on a few
    if bug == "one_in_300_up_a_bin":
        bins, w, u = _case("soft")
        good, moved = _buggy_sample_pdf(bins, w, u, None), _buggy_sample_pdf(bins, w, u, bug)
        differs = (good != moved)
        bad = SA.unaccounted(bins, w, u, moved)
        assert not bool((bad & ~differs).any())                  # no false alarm
        assert int((bad & differs).sum()) >= 0.9 * int(differs.sum()), (int((bad & differs).sum()), int(differs.sum()))


@pytest.mark.parametrize("family", ["soft", "peak"])
def test_missing_denom_branch_passes_the_flip_count_and_fails_the_accounting(family):
    """The point of the check in one assertion: a sample_pdf without its ``denom < 1e-5`` branch stays under the cap the GPU tests put on the
    flip count (the share of finite samples beyond 5e-6 of the oracle's: 5e-3 in test_sample_pdf_F4) -- and leaves samples unaccounted."""
    bins, w, u = _case(family)
    want = R.sample_pdf(bins, w, 128, False, u)
    got = _buggy_sample_pdf(bins, w, u, "no_denom_branch")
    finite = torch.isfinite(got)
    flips = float(((got - want).abs()[finite] > 5e-6).float().sum() / got.numel())
    bad = SA.unaccounted(bins, w, u, got)
    print(f"{family}: denom branch missing: old flip measure {flips:.4f} (cap 5e-3), unaccounted {float(bad.float().mean()):.4f}, "
          f"non-finite {int((~finite).sum())}")
    assert flips <= 5e-3 and int(bad.sum()) > 0, (flips, int(bad.sum()))


def test_nan_weight_row_is_skipped_and_finite_samples_in_it_are_flagged():
    bins, w, u = _case("soft", n=8)
    w[2, 7] = float("nan")
    s = R.sample_pdf(bins, w, 128, False, u)
    assert bool(torch.isnan(s[2]).all())                                     # the oracle: every sample of that row is NaN
    acc = SA.account(bins, w, u, s)
    assert bool(acc.nan_rows[2]) and int(acc.nan_rows.sum()) == 1 and int(acc.bad.sum()) == 0
    s[2, 11] = 4.0                                                           # a finite depth out of NaN weights
    bad = SA.unaccounted(bins, w, u, s)
    assert bool(bad[2, 11]) and int(bad.sum()) == 1


def test_fine_branch_bins_and_weights():
    """fine_account checks oracle.restate.fine_z's samples against mids(z_c) and weights_c[1:-1], whatever the two outer weights are."""
    for Sc, Nf in ((64, 128), (3, 1), (17, 40)):
        z_c = SA.sorted_depths(37, Sc, Sc)
        w_c = torch.cat([torch.rand(37, 1), SA.w_peak(37, Sc - 1, Sc), torch.rand(37, 1)], -1)
        for u in (None, SA.edge_uniforms(37, Nf, Sc + 1)):
            _, z_new = R.fine_z(z_c, w_c, Nf, u is None, u)
            assert int(SA.fine_account(z_c, w_c, u, z_new).bad.sum()) == 0


def test_check_is_fast():
    bins, w, u = _case("peak", n=4096)
    s = R.sample_pdf(bins, w, 128, False, u)
    dt = float("inf")
    for _ in range(3):                                                       # the best of three: the box may be busy
        t0 = time.perf_counter()
        bad = SA.unaccounted(bins, w, u, s)
        dt = min(dt, time.perf_counter() - t0)
    print(f"4096 x 128 samples checked in {dt * 1e3:.0f} ms")
    assert int(bad.sum()) == 0 and dt < 1.0, dt
