"""No GPU: track.fit_smoothness driven by the float64 oracle of tests/track_pairwise_oracle.py in place of the device read-out: labels sampled from the
chain at a known lam (and mu) are recovered within 4 of the fit's own standard errors - a statistical margin at fixed seeds, not a numerical one (the worst case seen
while the seeds were chosen lay 1.7 standard errors off) - labels that never change end at the bound, bad labels raise."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_pairwise_oracle as PW  # noqa: E402


def oracle_stats(logits, gate_logits, lam, mu):
    o = PW.pairwise(logits, lam) if gate_logits is None else PW.pairwise_gated(logits, gate_logits, lam, mu)
    return float(o['jump_abs'].sum()), (float(o['p_flip'].sum()) if gate_logits is not None else 0.0), o['log_z']


def labelled_recording(lam: float, W: int = 2000, C: int = 21):
    """The plain case of the fit tests (the GPU test of the default `stats` uses the lam = 1 one): 3 * randn logits, labels drawn from the chain at lam."""
    rng = np.random.default_rng(int(10 * lam))
    x = 3 * rng.standard_normal((W, C))
    return x, PW.sample_path(rng, x, lam)


@pytest.mark.parametrize('lam', [0.5, 1.0, 2.0])
def test_fit_recovers_lam(lam):
    from synchformer_amd.track import fit_smoothness
    x, y = labelled_recording(lam)
    f = fit_smoothness([(x, y)], iters=20, stats=oracle_stats)
    print(f'lam {lam}: fit {f.lam:.4f} +- {f.se_lam:.4f} ({(f.lam - lam) / f.se_lam:+.2f} se), J* {f.jumps_observed:.0f}, E[J] {f.jumps_expected:.3f}, '
          f'log-likelihood {f.log_likelihood:.2f}, {f.evaluations} evaluations')
    assert abs(f.lam - lam) <= 4 * f.se_lam and 0 < f.se_lam < 0.1 * lam
    assert not f.at_bound and f.mu is None and f.se_mu is None and f.flips_observed == f.flips_expected == 0
    assert f.jumps_observed == float(np.abs(np.diff(y)).sum())
    assert abs(f.jumps_expected - f.jumps_observed) <= 0.05 / f.se_lam              # the gradient at the fit: under 0.05 se of lam (d E[J] / d lam = -1 / se^2)
    assert f.log_likelihood < 0 and f.evaluations == 2 + 20 + 1 + 2
    # the log-likelihood is what it says: the labelled path's score minus log_z, and lower a little to either side of the fit
    e = x - PW.lse(x, axis=1)[:, None]
    score = e[np.arange(len(y)), y].sum() - f.lam * f.jumps_observed
    assert abs(f.log_likelihood - (score - PW.pairwise(x, f.lam)['log_z'])) <= 1e-8 * abs(score)
    for other in (f.lam - 3 * f.se_lam, f.lam + 3 * f.se_lam):
        assert e[np.arange(len(y)), y].sum() - other * f.jumps_observed - PW.pairwise(x, other)['log_z'] < f.log_likelihood


def test_fit_recovers_lam_and_mu_of_the_gated_chain():
    from synchformer_amd.track import fit_smoothness
    rng = np.random.default_rng(77)
    W, C = 1000, 21
    x, z = 3 * rng.standard_normal((W, C)), 2 * rng.standard_normal((W, 2))
    s = PW.sample_path(rng, x, 1.0, z, 2.0)
    f = fit_smoothness([(x, s % C, z, s // C)], gated=True, iters=16, sweeps=2, stats=oracle_stats)
    print(f'fit lam {f.lam:.4f} +- {f.se_lam:.4f} ({(f.lam - 1) / f.se_lam:+.2f} se), mu {f.mu:.4f} +- {f.se_mu:.4f} ({(f.mu - 2) / f.se_mu:+.2f} se), '
          f'F* {f.flips_observed:.0f}, E[F] {f.flips_expected:.3f}, {f.evaluations} evaluations')
    assert abs(f.lam - 1.0) <= 4 * f.se_lam and abs(f.mu - 2.0) <= 4 * f.se_mu and not f.at_bound
    assert 0 < f.se_lam < 0.1 and 0 < f.se_mu < 0.2
    assert f.flips_observed == float(np.abs(np.diff(s // C)).sum()) and f.jumps_observed == float(np.abs(np.diff(s % C)).sum())
    assert abs(f.jumps_expected - f.jumps_observed) <= 0.05 / f.se_lam and abs(f.flips_expected - f.flips_observed) <= 0.05 / f.se_mu     # both coordinates at rest


def test_several_recordings_add_up():
    """Two recordings: the observed and expected counts are the sums over both."""
    from synchformer_amd.track import fit_smoothness
    rng = np.random.default_rng(3)
    recs = []
    for W in (150, 90):
        x = 3 * rng.standard_normal((W, 9))
        recs.append((x, PW.sample_path(rng, x, 1.0)))
    f = fit_smoothness(recs, iters=12, stats=oracle_stats)
    assert f.jumps_observed == sum(float(np.abs(np.diff(y)).sum()) for _, y in recs) and not f.at_bound
    assert abs(sum(PW.pairwise(x, f.lam)['jump_abs'].sum() for x, _ in recs) - f.jumps_expected) <= 1e-9
    assert abs(f.lam - 1.0) <= 4 * f.se_lam


def test_labels_that_never_change_end_at_the_bound():
    from synchformer_amd.track import fit_smoothness
    x = 3 * np.random.default_rng(4).standard_normal((60, 9))
    f = fit_smoothness([(x, np.full(60, 4))], lam_max=8.0, iters=8, stats=oracle_stats)
    assert f.at_bound and f.lam_at_bound and f.lam == 8.0 and f.jumps_observed == 0 and f.jumps_expected >= 0
    z = np.random.default_rng(5).standard_normal((60, 2))
    g = fit_smoothness([(x, PW.sample_path(np.random.default_rng(6), x, 1.0), z, np.ones(60, np.int64))], gated=True, mu_max=6.0, iters=8, sweeps=1, stats=oracle_stats)
    assert g.at_bound and g.mu_at_bound and g.mu == 6.0 and not g.lam_at_bound and g.flips_observed == 0
    # labels that jump more than independent windows would: the likelihood falls from lam = 0 on
    wild = np.tile([0, 8], 30)
    h = fit_smoothness([(np.zeros((60, 9)), wild)], iters=8, stats=oracle_stats)
    assert h.lam_at_bound and h.lam == 0.0


def test_bad_labels_raise():
    from synchformer_amd.track import fit_smoothness
    x, z = np.zeros((10, 5)), np.zeros((10, 2))
    y = np.zeros(10, np.int64)
    bad = y.copy()
    bad[3] = 5
    neg = y.copy()
    neg[0] = -1
    for recs, kw in (([(x, bad)], {}), ([(x, neg)], {}), ([(x, y[:9])], {}), ([], {}), ([(x, y, z, y)], {}), ([(x, y)], dict(gated=True)),
                     ([(x, y, z, y + 2)], dict(gated=True)), ([(x, y, z[:9], y)], dict(gated=True)), ([(x, y, z, y[:9])], dict(gated=True)),
                     ([(x, bad, z, y)], dict(gated=True))):
        with pytest.raises(ValueError):
            fit_smoothness(recs, stats=oracle_stats, **kw)
