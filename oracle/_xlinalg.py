"""ORACLE (test infrastructure): the three dense factorisations the oracles call, dispatching on dtype.

float64 (and anything below it) goes to the NumPy function the oracles have always called -- the results are bitwise
those of np.linalg.  np.longdouble arrays, which LAPACK does not take, get a pure-NumPy version batched over the
leading axes, so that oracle/lds_closed_form.py and oracle/pca_closed_form.py can be run unchanged in extended
precision (tests/extended_ref.py) and serve as the reference the float64 oracle and the kernels are measured against.

The extended versions assume what every call site has: symmetric positive definite matrices (posterior precisions,
covariance blocks, Wishart scale matrices).
"""
import numpy as np

LD = np.longdouble
_NS_DONE = LD(2.0) ** -33          # a residual below this is squared to below 2^-66 < eps(long double) by one more step


def _is_ext(a):
    return np.asarray(a).dtype == LD and np.dtype(LD) != np.dtype(np.float64)


def inv(a):
    """np.linalg.inv; in long double the float64 inverse cast up and refined by Newton-Schulz steps X <- X (2 I - P X), each
    of which squares the residual I - P X: two steps always, more while the residual found was still above 2^-33."""
    if not _is_ext(a):
        return np.linalg.inv(a)
    a = np.asarray(a)
    n = a.shape[-1]
    if n == 0 or a.size == 0:
        return a.copy()
    X = np.linalg.inv(a.astype(np.float64)).astype(LD)
    eye = np.eye(n, dtype=LD)
    r = np.inf
    for step in range(12):
        R = eye - a @ X
        r = np.abs(R).sum(axis=-1).max()
        X = X + X @ R
        if step >= 1 and r < _NS_DONE:
            return X
    raise np.linalg.LinAlgError("Newton-Schulz refinement did not converge (residual %r)" % (r,))


def cholesky(a):
    """np.linalg.cholesky (lower factor); in long double the column-by-column recurrence, vectorised over the batch."""
    if not _is_ext(a):
        return np.linalg.cholesky(a)
    a = np.asarray(a)
    n = a.shape[-1]
    L = np.zeros_like(a)
    for j in range(n):
        d = a[..., j, j] - np.sum(L[..., j, :j] ** 2, axis=-1)
        if not np.all(d > 0):
            raise np.linalg.LinAlgError("Matrix is not positive definite")
        d = np.sqrt(d)
        L[..., j, j] = d
        if j + 1 < n:
            s = a[..., j + 1:, j] - np.einsum("...ik,...k->...i", L[..., j + 1:, :j], L[..., j, :j])
            L[..., j + 1:, j] = s / d[..., None]
    return L


def slogdet(a):
    """np.linalg.slogdet; in long double (sign = 1, 2 sum ln diag chol(a)) of a positive definite matrix."""
    if not _is_ext(a):
        return np.linalg.slogdet(a)
    L = cholesky(a)
    ld = 2.0 * np.sum(np.log(np.einsum("...ii->...i", L)), axis=-1)
    return np.ones_like(ld), ld
