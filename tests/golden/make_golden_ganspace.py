#!/usr/bin/env python3
"""GANSpace fixture generator (tests/golden/ganspace.npz).  Runs on the CPU of a development machine with a checkout of the reference
(cvlab-kaist/3DGAN-Inversion) and scikit-learn:

    python tests/golden/make_golden_ganspace.py REFERENCE_ROOT

Loads the reference's own ganspace/estimator.py by path (it needs only sklearn and numpy), fits PCAEstimator(n_components=24) on a seeded
float32 X [400, 24] -- Gaussian columns scaled 0.8^j, rotated by a random orthogonal matrix, plus a mean of about 3 -- and records X and what
get_components returns (components, stdev, var_ratio) with total_var.  Prints how far the float64 restatement of tests/support/pca_ref.py is from
the recorded values and the smallest relative gap between consecutive stdev (the conditioning of the components)."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SEED, S, D = 11, 400, 24


def make_x():
    rng = np.random.RandomState(SEED)
    g = rng.randn(S, D) * (0.8 ** np.arange(D))
    q, _ = np.linalg.qr(rng.randn(D, D))
    mean = 3.0 + 0.25 * rng.randn(D)
    return (g @ q.T + mean).astype(np.float32)


def main():
    ref_root = sys.argv[1]
    spec = importlib.util.spec_from_file_location('ref_ganspace_estimator', os.path.join(ref_root, 'ganspace', 'estimator.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    X = make_x()
    est = mod.PCAEstimator(n_components=D)
    est.fit(X)
    components, stdev, var_ratio = est.get_components()
    out = dict(X=X, components=np.asarray(components, dtype=np.float32), stdev=np.asarray(stdev, dtype=np.float32),
               var_ratio=np.asarray(var_ratio, dtype=np.float32), total_var=np.asarray(est.total_var, dtype=np.float32))
    path = os.path.join(HERE, 'ganspace.npz')
    np.savez(path, **out)
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'support'))
    from pca_ref import pca_ref
    r = pca_ref(X)
    print(f'{path}: {os.path.getsize(path)} bytes')
    print('float64 restatement vs estimator: components %.2e  stdev %.2e  var_ratio %.2e  total_var %.2e' % (
        np.abs(r['components'] - out['components']).max(), np.abs(r['stdev'] - out['stdev']).max(), np.abs(r['var_ratio'] - out['var_ratio']).max(),
        abs(r['total_var'] - float(out['total_var']))))
    sd = r['stdev']
    print('smallest relative gap between consecutive stdev: %.3f' % float(((sd[:-1] - sd[1:]) / sd[:-1]).min()))


if __name__ == '__main__':
    main()
