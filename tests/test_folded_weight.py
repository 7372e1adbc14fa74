"""K1's f64 pair weight with the source's mass folded into the polynomial (csrc/common.hpp: weight_far_folded) against the form
it replaces (weight_far), both emulated operation for operation with correctly rounded arithmetic and measured against the exact
term.  No GPU: the products are IEEE doubles, every FMA is formed exactly in rationals and rounded once, the v_rsq_f64 seed is
the exact reciprocal square root with a relative error drawn from +-2^-24.2 (the instruction's accuracy).

Three forms, as pair_batch takes them: no eps term (the sparse rule's far pairs, the softened twin), the eps term (the dense rule),
and the sparse rule's mixed batch, where a lane takes 2/3 eps or 0 by its own r^2 (>= 4: 0).  The new form must be as accurate as the
old one IN THE SAME RUN: max and rms error in ulp of the exact term at most 10 % above the old form's (the sampling scatter of
the maximum between runs of 60 000 pairs is ~6 %), and no bias: |mean signed error| <= 0.05 ulp.

The old eps form's own maximum is large (a cross term of up to 8 ulp near r^2 = 2^-16), so the relative bound alone would let the
new eps and mixed forms reach ~10 ulp.  The new form therefore also meets an ABSOLUTE maximum, ABS_MAX below, derived from its
operations and not from what it measures.  In units of u = 2^-53 relative (one rounding is <= 1 u; an error of c u is between c / 2
and c ulp of the result, by where the result lies in its binade):
    a = fl(y y)      delta <= 1 u moves y3 by +delta and the polynomial by -3/2 delta:                    0.5 u
    y3, s, w         one rounding each (t's and e's roundings are scaled by e <= 2^-23.2: < 2^-75):         3 u
    truncation       35/16 e^3 < 2^-68; (eps u)^2 / 6 < 2^-58:                                            < 0.1 u
    eps forms only   e' takes 2/3 eps y^3 for 2/3 eps r^-3: off by the seed's relative error d <= 2^-24.2 (x 3/2 in w):
                     eps y^3 d <= 2^-52 2^24 2^-24.2 = 2^-52.2 at r^2 = 2^-16:                             1.75 u
so <= 3.6 ulp without the eps term and <= 5.35 ulp with it, were every term at its worst at once."""
import math
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np
import pytest

getcontext().prec = 60
EPS = 2.0 ** -52
N = 60000


def fma(a, b, c):
    """fl(a * b + c): exact in rationals, rounded once (int / int division is correctly rounded)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def old_weight(r2, mj, y, eps):
    """pair_math<double>::weight_far: eps None = weight_far<false>, else weight_far<true> with that eps (DBL_EPSILON or 0)."""
    a = y * y
    e = fma(-r2, a, 1.0)
    y3 = a * y
    p = fma(e, 1.875, 1.5)
    g = p * e if eps is None else fma(p, e, -(eps * y3))
    my = mj * y3
    return fma(my, g, my)


EPS23 = 2.0 / 3.0 * EPS
ABS_MAX = {"no_eps": 3.6, "eps": 5.35, "mixed": 5.35}   # ulp: the worst case of the new form's own operations (module docstring)


def new_weight(r2, mj, y, keps):
    """pair_math<double>::weight_far_folded: keps None = <false>, else <true> with that constant (2/3 eps or 0)."""
    m15, m1875 = 1.5 * mj, 1.875 * mj
    a = y * y
    e = fma(-r2, a, 1.0)
    y3 = a * y
    if keps is not None:
        e = fma(-keps, y3, e)
    t = fma(e, m1875, m15)
    s = fma(t, e, mj)
    return y3 * s


def samples(seed):
    rng = np.random.default_rng(seed)
    r2 = 2.0 ** rng.uniform(-16, 12, N)
    mj = 10.0 ** rng.uniform(-3, 3, N)
    y = (1.0 / np.sqrt(r2)) * (1.0 + rng.uniform(-1, 1, N) * 2.0 ** -24.2)
    return r2, mj, y


def ulps(w, exact):
    return float((Decimal(w) - exact) / Decimal(math.ulp(float(exact))))


def stats(errs):
    e = np.asarray(errs)
    return np.abs(e).max(), math.sqrt(np.mean(e * e)), e.mean()


@pytest.mark.parametrize("form", ["no_eps", "eps", "mixed"])
def test_folded_weight_is_as_accurate_as_the_form_it_replaces(form):
    r2s, mjs, ys = samples({"no_eps": 11, "eps": 12, "mixed": 13}[form])
    old, new = [], []
    for r2, mj, y in zip(r2s.tolist(), mjs.tolist(), ys.tolist()):
        r3 = Decimal(r2) * Decimal(r2).sqrt()
        if form == "no_eps":
            exact = Decimal(mj) / r3
            wo, wn = old_weight(r2, mj, y, None), new_weight(r2, mj, y, None)
        else:
            exact = Decimal(mj) / (r3 + Decimal(EPS))
            far = form == "mixed" and r2 >= 4.0   # a lane's own choice in a mixed batch: the eps term below r^2 = 4, 0 from there
            wo, wn = old_weight(r2, mj, y, 0.0 if far else EPS), new_weight(r2, mj, y, 0.0 if far else EPS23)
            if far:  # the choice of 0 gives the bits of the form without the term
                assert wo == old_weight(r2, mj, y, None) and wn == new_weight(r2, mj, y, None)
        old.append(ulps(wo, exact))
        new.append(ulps(wn, exact))
    (omax, orms, omean), (nmax, nrms, nmean) = stats(old), stats(new)
    print(f"{form}: old max {omax:.3f} rms {orms:.3f} mean {omean:+.4f} ulp | new max {nmax:.3f} rms {nrms:.3f} mean {nmean:+.4f} ulp")
    assert nmax <= 1.10 * omax, (nmax, omax)
    assert nmax <= ABS_MAX[form], (nmax, ABS_MAX[form])
    assert nrms <= 1.10 * orms, (nrms, orms)
    assert abs(nmean) <= 0.05, nmean


def test_padding_record_adds_zero():
    """A zero-mass padding record has constants 0 and weight y3 * 0 = 0 in both forms."""
    assert new_weight(9.0, 0.0, 1 / 3, EPS23) == 0.0 and new_weight(9.0, 0.0, 1 / 3, None) == 0.0
