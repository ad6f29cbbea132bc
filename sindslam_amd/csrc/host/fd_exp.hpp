// exp, DEFINED (not taken from a maths library on either side): reduction x = k ln2 + r with k = rint(x / ln2) (ln2 split in two as in fdlibm's e_exp.c), fdlibm's
// polynomial c = r - r^2 (P1 + ...), y = 1 - ((lo - r c / (2 - c)) - hi) for every k (fdlibm's separate k = 0 form is not used), then an exact scaling by 2^k (ldexp).
// Only add, mul, div, rint, compares and that scaling.  exp(0) = 1 exactly, NaN gives NaN, above 709.78 +inf, below -745.2 zero.  Used by sim3_opt.hpp (where the
// choice is argued, point 5 of its header) and by occmap.hpp.
#pragma once
#include <cfloat>
#include <cmath>
#include "peac_fit.hpp"                                              // SIND_HD

namespace sind {

SIND_HD inline double s3_exp(double x) {
    if (!(x == x)) return x;
    if (x > 709.782712893384) return DBL_MAX * 2.0;
    if (x < -745.2) return 0.0;
    const double ln2HI = 6.93147180369123816490e-01, ln2LO = 1.90821492927058770002e-10, invln2 = 1.44269504088896338700e+00;
    const double P1 = 1.66666666666666019037e-01, P2 = -2.77777777770155933842e-03, P3 = 6.61375632143793436117e-05, P4 = -1.65339022054652515390e-06, P5 = 4.13813679705723846039e-08;
    const double fn = __builtin_rint(x * invln2);
    const double hi = x - fn * ln2HI, lo = fn * ln2LO;
    const double r = hi - lo, t = r * r;
    const double c = r - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))));
    const double y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi);
    return ldexp(y, (int)fn);
}

}  // namespace sind
