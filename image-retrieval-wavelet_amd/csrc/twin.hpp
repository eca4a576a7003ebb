// What the kernels' translation units and their host twins (host_*.cpp: plain C++, no device pass) both need: the error
// report, the function qualifier of code compiled for both sides, and the limits and checks the two sides answer alike.
// No HIP header is included, so a plain C++ compiler can take this file; common.hpp includes it for the device side.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/wvhash.h"

#ifdef __HIP__
#define WV_HD __host__ __device__ inline
#else
#define WV_HD inline
#endif

namespace wv {

void set_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));

#define WV_FAIL(code, ...)          \
    do {                            \
        ::wv::set_error(__VA_ARGS__); \
        return (code);              \
    } while (0)

#define WV_REQUIRE(cond, ...)                      \
    do {                                           \
        if (!(cond)) WV_FAIL(WV_EINVAL, __VA_ARGS__); \
    } while (0)

constexpr int kMaxImageSide = 16384;    // H, W of an image of wv_image_size, wv_colour_jitter and wv_lift_images

// The n byte ranges [first(i), end(i)) must not overlap: sorted by first byte, each must end before the next begins.
// -> false, or true with `a` the range that runs into `b`.
template <class First, class End>
inline bool ranges_overlap(int n, First first, End end, int *a, int *b)
{
    std::vector<int> order(n);
    for (int i = 0; i < n; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](int x, int y) { return first(x) < first(y); });
    for (int j = 1; j < n; ++j)
        if (end(order[j - 1]) > first(order[j])) {
            *a = order[j - 1], *b = order[j];
            return true;
        }
    return false;
}

}  // namespace wv
