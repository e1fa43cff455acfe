"""Float64 numpy restatement of pfm_frechet_grad (probaforms_amd/metrics/csrc/pf_metrics.h): the Frechet distance of two samples as
given, its parts, the eigenvalues of the real-side M, the ranks kept by the cut and both samples' row gradients, through
np.linalg.eigh; and a second, independent route for non-singular inputs through scipy.linalg.sqrtm and np.linalg.solve.  Test
helper, not product code."""
import numpy as np

U53 = 2.0 ** -53


def data(nr, nf, d, seed=0):
    """real sample: normal @ (I + 0.3 normal / sqrt(d)) + 1; fake sample: 0.8 normal + 0.3"""
    rng = np.random.RandomState(1000 * d + 7 * nr + nf + seed)
    Xr = rng.normal(size=(nr, d)) @ (np.eye(d) + 0.3 * rng.normal(size=(d, d)) / np.sqrt(d)) + 1.0
    Xf = 0.8 * rng.normal(size=(nf, d)) + 0.3
    return Xr, Xf


def moments(X):
    """np.cov(rowvar=False), ddof 1, as a [d, d] matrix also for d = 1"""
    d = X.shape[1]
    return X.mean(axis=0), np.cov(X, rowvar=False).reshape(d, d)


def sqrt_psd(A):
    """A^(1/2) from the eigen-decomposition of A with the eigenvalues clipped at 0 (fd.trace_sqrtm's S)"""
    w, V = np.linalg.eigh(A)
    return (V * np.sqrt(np.clip(w, 0.0, None))) @ V.T


def route(A, B, rcond):
    """one route: S = A^(1/2), M = sym(S B S) -> (tr sqrt, eigenvalues of M ascending, kept, G = I - S M^(-1/2)_cut S = dFD/dB)"""
    S = sqrt_psd(A)
    M = S @ B @ S
    lam, V = np.linalg.eigh((M + M.T) * 0.5)
    trs = float(np.sum(np.sqrt(np.clip(lam, 0.0, None))))
    lmax = lam[-1]
    keep = (lam > rcond * lmax) if lmax > 0 else np.zeros(lam.shape, dtype=bool)
    c = np.zeros_like(lam)
    c[keep] = 1.0 / np.sqrt(lam[keep])
    G = np.eye(len(lam)) - S @ ((V * c) @ V.T) @ S
    return trs, lam, int(keep.sum()), G


def row_gradient(X, mu, mu_other, G):
    n = X.shape[0]
    return (2.0 / n) * (mu - mu_other)[None, :] + (2.0 / (n - 1)) * (X - mu[None, :]) @ ((G + G.T) * 0.5)


def value_grad(Xr, Xf, rcond=None):
    """-> dict(value, parts [5], eig [d], rank [2], grad_r [nr, d], grad_f [nf, d], scale = |dmu|^2 + tr C_r + tr C_f)"""
    d = Xr.shape[1]
    if rcond is None:
        rcond = d * 2.0 ** -52
    mr, Cr = moments(Xr)
    mf, Cf = moments(Xf)
    trs, lam, kept, Gf = route(Cr, Cf, rcond)
    _, lam_sw, kept_sw, Gr = route(Cf, Cr, rcond)
    dm2 = float(np.sum((mr - mf) ** 2))
    scale = dm2 + np.trace(Cr) + np.trace(Cf)
    value = scale - 2.0 * trs
    return dict(value=value, parts=np.array([value, dm2, np.trace(Cr), np.trace(Cf), trs]), eig=lam, eig_swapped=lam_sw,
                rank=np.array([kept, kept_sw]), grad_r=row_gradient(Xr, mr, mf, Gr), grad_f=row_gradient(Xf, mf, mr, Gf),
                scale=float(scale), Gr=Gr, Gf=Gf, mean=np.stack([mr, mf]), cov=np.stack([Cr, Cf]))


def value_of(Xr, Xf):
    return value_grad(Xr, Xf)["value"]


def independent(Xr, Xf):
    """the second route, for non-singular covariances: tr sqrtm(C_r C_f) by scipy's Schur method, and with R = sqrtm(C_r C_f),
    d tr R / dC_f = (1/2) R^-1 C_r, so G_f = I - solve(R, C_r), G_r = I - solve(sqrtm(C_f C_r), C_f)"""
    from scipy.linalg import sqrtm
    mr, Cr = moments(Xr)
    mf, Cf = moments(Xf)
    d = len(mr)
    R = np.real(sqrtm(Cr @ Cf)).reshape(d, d)
    R2 = np.real(sqrtm(Cf @ Cr)).reshape(d, d)
    Gf = np.eye(d) - np.linalg.solve(R, Cr)
    Gr = np.eye(d) - np.linalg.solve(R2, Cf)
    scale = float(np.sum((mr - mf) ** 2) + np.trace(Cr) + np.trace(Cf))
    return dict(value=scale - 2.0 * float(np.trace(R)), grad_r=row_gradient(Xr, mr, mf, Gr), grad_f=row_gradient(Xf, mf, mr, Gf),
                scale=scale)


def standardized(Xr, Xf):
    """StandardScaler fitted on the real sample (population std; 0 becomes 1), applied to both, in numpy"""
    mu, sd = Xr.mean(axis=0), Xr.std(axis=0)
    sd = np.where(sd == 0, 1.0, sd)
    return (Xr - mu) / sd, (Xf - mu) / sd
