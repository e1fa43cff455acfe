#!/usr/bin/env python3
"""Generate tests/golden/twosample_*.npz: the permutation two-sample tests energy_test and mmd_test, computed by the float64
numpy / scipy restatement tests/twosample_numpy.py (Philox4x32-10 labellings by stable argsort, scipy's cdist, einsum).  Needs
numpy and scipy only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_twosample.py

The reference has no such test.  One case, mmd_reference, takes its statistic and its median from the reference's own
probaforms/metrics/mmd.py (mmd_calc, and the np.median(pairwise_distances(...)) that mmd_calc computes inside); it is made
only where a checkout of the reference and sklearn are at hand, and is otherwise left as committed:

    PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_twosample.py --reference

Per case the file holds X, Y, seed (np.random.seed before the call), n_permutations, standardize (whether the values are
those of the samples scaled by the real sample's StandardScaler), next (np.random.random() after a call: each call makes the
one seed draw) and, for energy_test as energy_* and for mmd_test as mmd_*:
  statistic   of the samples as given          null  [n_permutations] of the drawn labellings, labelling p at index p
  pvalue      (1 + #{null >= statistic}) / (1 + n_permutations)
and median, the pooled median distance mmd_test takes its bandwidth from.

A fixture's p-value must be a matter of counting: the generator asserts that every null value either belongs to a labelling
equal to the observed one (its sum is then the observed sum, bit for bit, on any implementation whose sums depend on the labels
alone) or lies further from the statistic than the two values' tolerances 1e-12 A / (nr nf)^2 together.
The continuous samples are rounded to multiples of 1/64 so that the files stay small.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import twosample_numpy as tn  # noqa: E402


def one(Xs, Ys, seed, P, kind, gamma):
    np.random.seed(seed)
    o = tn.test(Xs, Ys, P, kind, gamma)
    N, nr = len(Xs) + len(Ys), len(Xs)
    L = tn.labels(o["key"], 0, P, N, nr)
    same = (L == tn.observed(N, nr)[None]).all(axis=1)
    gap = np.abs(o["null"] - o["statistic"])
    assert (same | (gap > o["bound"][1:] + o["bound"][0])).all(), "a null value within the tolerance of the statistic"
    assert o["pvalue"] == (1 + int((o["null"] >= o["statistic"]).sum())) / (1 + P)
    return o


def case(X, Y, seed, P, standardize=False, median=None, mmd_statistic=None):
    Xs, Ys = tn.standardize(X, Y) if standardize else (X, Y)
    med = tn.median(Xs, Ys) if median is None else median
    e = one(Xs, Ys, seed, P, tn.ENERGY, 0.0)
    m = one(Xs, Ys, seed, P, tn.GAUSS, 1.0 / (2 * med ** 2))
    assert e["next"] == m["next"] and e["key"] == m["key"]
    if mmd_statistic is not None:                 # the reference's value in place of the restatement's, which must agree
        assert abs(mmd_statistic - m["statistic"]) <= m["bound"][0]
        m["statistic"] = np.float64(mmd_statistic)
        assert m["pvalue"] == tn.pvalue(m["statistic"], m["null"])
    return dict(X=X, Y=Y, seed=seed, n_permutations=P, standardize=standardize, median=med, next=e["next"],
                energy_statistic=e["statistic"], energy_null=e["null"], energy_pvalue=e["pvalue"],
                mmd_statistic=m["statistic"], mmd_null=m["null"], mmd_pvalue=m["pvalue"])


def grid(A):
    return np.round(A * 64) / 64


def cases():
    """-> {name: the file's arrays}; numpy and scipy only"""
    rng = np.random.default_rng(1818)
    out = {}
    out["shift_130_93_d3"] = case(grid(rng.normal(size=(130, 3))), grid(rng.normal(0.6, 1.0, size=(93, 3))), seed=71, P=199)
    out["equal_130_93_d3"] = case(grid(rng.normal(size=(130, 3))), grid(rng.normal(size=(93, 3))), seed=72, P=199)
    out["integer_65_63_d1"] = case(rng.integers(-1000, 1001, size=(65, 1)).astype(np.float64),
                                   rng.integers(-900, 1101, size=(63, 1)).astype(np.float64), seed=73, P=99)
    out["tiny_1_2_d1"] = case(np.array([[0.25]]), np.array([[-1.5], [2.0]]), seed=74, P=20)
    real = np.concatenate([rng.normal(-4, 1, size=(60, 3)), rng.normal(4, 1, size=(60, 3))]) * [5.0, 0.1, 1.0] + [100.0, 0, -7]
    fake = np.concatenate([rng.normal(-3, 1, size=(50, 3)), rng.normal(5, 1, size=(50, 3))]) * [5.0, 0.1, 1.0] + [100.0, 0, -7]
    out["clusters_standardized"] = case(grid(real), grid(fake), seed=75, P=99, standardize=True)
    return out


def reference_case():
    """mmd_reference: the statistic and the median of the reference's mmd_calc"""
    from probaforms.metrics import mmd as ref_mmd  # the reference
    from sklearn import metrics
    assert not getattr(sys.modules["probaforms"], "__probaforms_amd__", False), "must import the reference"
    rng = np.random.default_rng(1819)
    X, Y = grid(rng.normal(size=(70, 4))), grid(rng.normal(0.25, 1.3, size=(58, 4)))
    med = np.median(metrics.pairwise_distances(np.concatenate((X, Y), axis=0)))        # mmd_calc's median_distance
    return {"mmd_reference": case(X, Y, seed=76, P=99, median=med, mmd_statistic=ref_mmd.mmd_calc(X, Y))}


def main():
    made = cases()
    if "--reference" in sys.argv[1:]:
        made.update(reference_case())
    for name, arrays in made.items():
        path = os.path.join(HERE, "twosample_%s.npz" % name)
        np.savez_compressed(path, **arrays)
        print(name, arrays["X"].shape, arrays["Y"].shape, "energy", arrays["energy_statistic"], arrays["energy_pvalue"],
              "mmd", arrays["mmd_statistic"], arrays["mmd_pvalue"], os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
