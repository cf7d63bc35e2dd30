// series_screen_rule.h -- the screen level of the screened RGB8 series kernel
// (series_v2_screen.h) for a threshold tau.  Plain C++ with no HIP in it, so
// that a host test can compile the rule itself (tests/test_screen_bound.py).
#pragma once

#include <cmath>

namespace dips {

// With J = max + min of a pixel's channels, 255 * |dI2| = |dJ| + err,
// |err| < 1.1e-4 (series_v2_frame.h), and a pixel is selected when
// |dI| = |dI2| / 2 > tau, i.e. 255 * |dI2| > 510 * tau.  So no pixel with
// |dJ| <= s is selected for the largest integer s with s + 3e-4 < 510 * tau
// (3e-4: the error bound with room to spare); -1 where even |dJ| = 0 could be
// (tau = 0), 510 = the largest |dJ| there is.
inline int series_screen_level(float tau) {
    const double lim = 510.0 * (double)tau - 3e-4;  // s < lim
    if (!(lim > 0.0)) return -1;
    if (lim > 510.0) return 510;
    const double c = std::ceil(lim);
    return (int)c - 1;  // the largest integer below lim (lim itself when it is whole: excluded)
}

}  // namespace dips
