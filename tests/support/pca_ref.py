"""Float64 restatement of the PCA the GANSpace estimator computes (sklearn PCA with svd_solver='full', then the estimator's re-sorting by
projected standard deviation): centre, ddof-0 covariance, eigh, descending, every component signed so that its largest-magnitude entry (the
first of equals) is positive.  What tests/test_ganspace_cpu.py checks against the recorded estimator output (tests/golden/ganspace.npz) and
what the GPU tests compare inv3d_amd.ganspace against."""
import numpy as np


def sign_rows(v: np.ndarray) -> np.ndarray:
    """Rows of v, each multiplied by the sign of its largest-magnitude entry (np.argmax takes the first of equals)."""
    idx = np.argmax(np.abs(v), axis=1)
    s = np.sign(v[np.arange(v.shape[0]), idx])
    s[s == 0] = 1.0
    return v * s[:, None]


def sym_eig_ref(a: np.ndarray):
    """(evals descending, evecs as signed rows) of the symmetric matrix a, in float64."""
    lam, vec = np.linalg.eigh(np.asarray(a, dtype=np.float64))
    order = np.argsort(-lam, kind='stable')
    return lam[order], sign_rows(vec[:, order].T)


def pca_ref(X: np.ndarray, n_components=None) -> dict:
    X = np.asarray(X, dtype=np.float64)
    mean = X.mean(axis=0)
    Xc = X - mean
    cov = Xc.T @ Xc / X.shape[0]
    lam, comp = sym_eig_ref(cov)
    K = X.shape[1] if n_components is None else int(n_components)
    total_var = float(np.trace(cov))
    stdev = np.sqrt(np.clip(lam[:K], 0.0, None))
    return dict(components=comp[:K], stdev=stdev, var_ratio=stdev ** 2 / total_var, total_var=total_var, mean=mean, cov=cov, evals=lam)
