"""ORACLE (test infrastructure): digamma and gammaln, dispatching on dtype as oracle/_xlinalg.py does.

float64 (and anything below it) goes to scipy.special -- the results are bitwise those the oracles have always had.
np.longdouble gets a pure-NumPy version, vectorised: the recurrence upwards until x >= 30,
    psi(x) = psi(x + m) - sum_{j<m} 1 / (x + j),      ln|Gamma(x)| = ln Gamma(x + m) - ln|x (x + 1) ... (x + m - 1)|
(one logarithm of the product, not m logarithms), then the asymptotic series with the Bernoulli numbers B_2 ... B_30,
    psi(x)      ~ ln x - 1 / (2 x) - sum_k B_2k / (2k x^2k)
    ln Gamma(x) ~ (x - 1/2) ln x - x + 1/2 ln 2 pi + sum_k B_2k / (2k (2k - 1) x^(2k-1)),
whose first omitted term is below 1e-36 at x = 30.  The two dominant products and sums of ln Gamma (where ln Gamma(x + m)
and the logarithm of the product cancel for small x) are formed as unevaluated head + tail pairs, so that the cancellation
does not cost the digits the lower bound's small-argument terms need.

Negative non-integer arguments go through the recurrence only -- no reflection formula, which is what the kernels use: the
reference's method stays different from theirs.  Poles (0, -1, -2, ...) give NaN (digamma) and +inf (gammaln), +inf gives
+inf, NaN gives NaN.  tests/test_extended_ref_cpu.py checks both functions against mpmath at 40 digits; this module does
not import it.
"""
import numpy as np
import scipy.special as _sp

LD = np.longdouble
_UP_TO = 30
_RECURRENCE_MAX = 1 << 20       # a negative argument below this would walk more than a million steps: refused

# B_2, B_4, ..., B_30 as exact rationals (numerator, denominator)
_BERNOULLI = ((1, 6), (-1, 30), (1, 42), (-1, 30), (5, 66), (-691, 2730), (7, 6), (-3617, 510), (43867, 798), (-174611, 330),
              (854513, 138), (-236364091, 2730), (8553103, 6), (-23749461029, 870), (8615841276005, 14322))
_HALF_LN_2PI = LD("0.918938533204672741780329736405617639861397473637783412817151540482765695927260397694743298635954197622")
_PI = LD("3.14159265358979323846264338327950288419716939937510582097494459")
_SPLIT = LD(2.0) ** 32 + 1      # Dekker's splitter for a 64-bit significand


def _is_ext(x):
    return np.asarray(x).dtype == LD and np.dtype(LD) != np.dtype(np.float64)


def _ratio(num, den):
    """num / den in long double from exact integers (the numerators above exceed 2^53: no float64 on the way)"""
    return LD(str(num)) / LD(str(den))


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    p = a * b
    ta = _SPLIT * a; ah = ta - (ta - a); al = a - ah
    tb = _SPLIT * b; bh = tb - (tb - b); bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _log2(x):
    """ln x as a head + tail pair: one Newton step on exp, l1 = l0 + (x exp(-l0) - 1), the correction kept as the tail.  The
    tail inherits the rounding of exp(-l0), about 2^-64 absolute, so the pair is good to about 1e-19 absolute whatever |ln x|
    is: a gain only where |ln x| >> 1 (half an ulp of ln 29! is 3.5e-18), which is the logarithm of the large product it is
    used for.  The mpmath grid of tests/test_extended_ref_cpu.py is what vouches for the result."""
    l0 = np.log(x)
    e = np.exp(-l0)
    p, pe = _two_prod(x, e)
    return l0, (p - 1.0) + pe


def _prepare(x):
    x = np.array(x, dtype=LD, ndmin=1)
    pole = (x <= 0) & (x == np.floor(x))
    bad = ~np.isfinite(x) | pole
    if np.any(~bad & (x < -_RECURRENCE_MAX)):
        raise ValueError("long-double recurrence refused below %d" % -_RECURRENCE_MAX)
    return x, pole, bad


def _digamma_ext(x0):
    x, pole, bad = _prepare(x0)
    work = np.where(bad, LD(_UP_TO), x)
    r = np.zeros_like(work)
    while True:
        low = work < _UP_TO
        if not low.any():
            break
        safe = np.where(low, work, LD(1))
        r = np.where(low, r - 1.0 / safe, r)
        work = np.where(low, work + 1.0, work)
    f = 1.0 / (work * work)
    ser = np.zeros_like(work)
    for k in range(len(_BERNOULLI), 0, -1):
        num, den = _BERNOULLI[k - 1]
        ser = f * (_ratio(num, den * 2 * k) + ser)
    out = r + (np.log(work) - 0.5 / work - ser)
    out = np.where(pole | np.isnan(x) | (x == -np.inf), LD(np.nan), np.where(x == np.inf, LD(np.inf), out))
    return out


def _gammaln_ext(x0):
    x, pole, bad = _prepare(x0)
    work = np.where(bad, LD(_UP_TO), x)
    prod = np.ones_like(work)           # |x (x + 1) ... (x + m - 1)|, folded into (lp, lpe) before it can overflow
    lp = np.zeros_like(work); lpe = np.zeros_like(work)
    perr = np.zeros_like(work)          # relative error of prod, first order: sum of the error of each product / the product
    while True:
        low = work < _UP_TO
        if not low.any():
            break
        big = np.abs(prod) > LD(1e300)
        if big.any():
            h, t = _log2(np.where(big, prod, LD(1)))
            lp, e = _two_sum(lp, h)
            lpe = lpe + e + t + np.where(big, perr, 0.0)
            prod = np.where(big, LD(1), prod); perr = np.where(big, LD(0), perr)
        fac = np.where(low, np.abs(work), LD(1))
        p, pe = _two_prod(prod, fac)
        perr = perr + pe / p
        prod = p
        work = np.where(low, work + 1.0, work)
    h, t = _log2(prod)
    lp, e = _two_sum(lp, h)
    lpe = lpe + e + t + perr
    # Stirling at work >= 30, head + tail: (work - 1/2) ln work - work + 1/2 ln 2 pi + series
    lw, lwe = _log2(work)
    a, ae = _two_prod(work - 0.5, lw)
    ae = ae + (work - 0.5) * lwe
    s, se = _two_sum(a, -work)
    s2, se2 = _two_sum(s, _HALF_LN_2PI)
    rx = 1.0 / work
    f = rx * rx
    ser = np.zeros_like(work)
    for k in range(len(_BERNOULLI), 0, -1):
        num, den = _BERNOULLI[k - 1]
        ser = _ratio(num, den * 2 * k * (2 * k - 1)) + f * ser
    ser = ser * rx
    tail = ae + se + se2 + ser
    d, de = _two_sum(s2, -lp)
    out = d + (de + tail - lpe)
    out = np.where(pole | (x == np.inf) | (x == -np.inf), LD(np.inf), np.where(np.isnan(x), LD(np.nan), out))
    return out


def _wrap(fn_ext, fn64, x):
    if not _is_ext(x):
        return fn64(x)
    out = fn_ext(x)
    return out.reshape(np.shape(x)) if np.ndim(x) else out[0]


def digamma(x):
    """scipy.special.digamma; in long double the recurrence to x >= 30 and the asymptotic series."""
    return _wrap(_digamma_ext, _sp.digamma, x)


def gammaln(x):
    """scipy.special.gammaln (ln |Gamma(x)|); in long double the recurrence to x >= 30 and Stirling's series."""
    return _wrap(_gammaln_ext, _sp.gammaln, x)


def ln2pi(like):
    """ln 2 pi in the dtype of `like`: np.log(2.0 * np.pi) as the oracles have always formed it, or its long-double value"""
    return np.log(2.0 * _PI) if _is_ext(like) else np.log(2.0 * np.pi)


def lnpi(like):
    return np.log(_PI) if _is_ext(like) else np.log(np.pi)
