"""Design effect of scan = "wave" on a success rate: the 64 ladders of a wavefront share their generator picks, so the
syndromes of a wavefront are not independent samples.  For toric L = 5 and L = 9, on scan = "wave" and (the control) scan = "random":
128 wavefronts of fresh syndromes, fixed-length runs with every step recorded (tops_burn = 0), and

  deff_success  = variance of the 128 wavefront success means / (p (1 - p) / 64)     (1: independent syndromes; 64: one per wavefront)
  icc_success   = (deff_success - 1) / 63                                             the intra-wavefront correlation of the success indicator
  deff_tops0 / icc_tops0: the same for tops0 (the count of top-chain arrivals at the bottom)

One JSON line.  Usage: python tools/design_effect.py [--wavefronts 128]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mcmc-qec-toric-rl_amd")]

import numpy as np  # noqa: E402

from qecmc import harness  # noqa: E402

CASES = [dict(L=5, Nc=5, p=0.12, steps=10000), dict(L=9, Nc=8, p=0.12, steps=20000)]


def _deff(x, K):
    x = np.asarray(x, dtype=np.float64)
    g = x.reshape(K, 64).mean(axis=1)
    v = x.var(ddof=1)
    d = float(g.var(ddof=1) / (v / 64)) if v > 0 else float("nan")
    return d, (d - 1) / 63


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wavefronts", type=int, default=128)
    a = ap.parse_args()
    K = a.wavefronts
    rows = []
    for c in CASES:
        for scan in ("wave", "random"):
            params = {"code": "toric", "size": c["L"], "p_error": c["p"], "noise": "depolarizing", "Nc": c["Nc"]}
            out = harness.generate(params, 64 * K, seed=11, rng=np.random.default_rng([11, c["L"]]), steps=c["steps"], conv_criteria=None,
                                   tops_burn=0, scan=scan)
            ds, rs = _deff(out["success"], K)
            dt, rt = _deff(out["tops0"], K)
            m = out["metrics"]
            rows.append(dict(code="toric", L=c["L"], Nc=c["Nc"], p=c["p"], steps=c["steps"], scan=scan, syndromes=64 * K,
                             success_rate=m["success_rate"], err=m["success_rate_err"], err_binomial=m["success_rate_err_binomial"],
                             err_method=m["success_rate_err_method"], deff_success=ds, icc_success=rs, deff_tops0=dt, icc_tops0=rt))
    print(json.dumps(dict(tool="design_effect", wavefronts=K, rows=rows)))


if __name__ == "__main__":
    main()
