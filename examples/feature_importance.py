#!/usr/bin/env python3
"""Which biomarker predicts sensitivity to which drug (doseresponse/feature_importance.py:39-54), with uncertainty: the chain of
examples/doseresponse_row_features.py, whose run_gibbs returns the sampled feature embeddings "U" (S,F,K) beside W and V,
then posterior_feature_association on the GPU.  For every (feature, drug) pair and kept sample, the per-row AUC of the
sampled curves is regressed on the per-row feature probability w_i . u_f; the table lists the strongest positive
(resistant: a higher AUC with the feature) and negative (sensitive) associations by the posterior mean of r, with the 90 %
interval and P(r > 0) over the samples, beside the reference's plug-in r of posterior means."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from doseresponse_row_features import main as fit                                     # noqa: E402
from functionalmf_amd.utils import posterior_feature_association                      # noqa: E402


def main(ntop=5, verbose=True, **kw):
    results, _ = fit(verbose=False, **kw)
    out = posterior_feature_association(results["W"], results["V"], results["U"], which="auc", stats=("r", "slope"), q=(5, 95))
    r, om = out["r"], out["of_means"]
    # the two filters of feature_importance.py:50, then the order of its lines 62 and 65
    keep = (om["sd_x"][:, None] >= 0.05) & (om["sd_y"][None, :] >= 0.05) & (out["defined"] > 0)
    score = np.where(keep, r["mean"], np.nan)
    order = [k for k in np.argsort(score, axis=None) if not np.isnan(score.flat[k])]
    F, M = score.shape
    rows = []
    for title, ks in (("resistant", order[::-1][:ntop]), ("sensitive", order[:ntop])):
        for k in ks:
            f, j = divmod(int(k), M)
            rows.append((title, f, j, r["mean"][f, j], r["quantiles"][0, f, j], r["quantiles"][1, f, j], r["prob_positive"][f, j],
                         om["r"][f, j], out["slope"]["mean"][f, j]))
    if verbose:
        print("%d samples, %d features x %d drugs, %d pairs pass the sd >= 0.05 filters" % (out["nsamples"], F, M, int(keep.sum())))
        print("%-10s %7s %5s %8s %17s %8s %10s %8s" % ("", "feature", "drug", "mean r", "90 % interval", "P(r>0)", "plug-in r", "slope"))
        for title, f, j, m, lo, hi, p, plug, slope in rows:
            print("%-10s %7d %5d %8.3f   [%6.3f, %6.3f] %8.2f %10.3f %8.3f" % (title, f, j, m, lo, hi, p, plug, slope))
    return out, rows


if __name__ == "__main__":
    main()
