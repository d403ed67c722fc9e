// Host-side helpers that need no HIP header: the error channel and the integer helpers.  common.h includes this for every unit of the
// library; plain C++ that includes it alone (conv_plan.h, tests/host/conv_plan_check.cpp) supplies its own pasta::fail.
#ifndef PASTA_HOST_COMMON_H
#define PASTA_HOST_COMMON_H
#include <stdint.h>

#if defined(__HIPCC__)
#define PASTA_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define PASTA_HD inline
#endif

namespace pasta {

// Thread-local error text returned by pasta_last_error().
char* error_buffer();
int   fail(const char* fmt, ...);

#define PASTA_CHECK(cond, ...)                         \
    do {                                               \
        if (!(cond)) return ::pasta::fail(__VA_ARGS__); \
    } while (0)

static inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// floor(a / b) for b > 0 and any sign of a.
PASTA_HD int floordiv(int a, int b) {
    int q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}
// a mod b in [0, b) for b > 0.
PASTA_HD int posmod(int a, int b) {
    int r = a % b;
    return r < 0 ? r + b : r;
}

}  // namespace pasta

#endif  // PASTA_HOST_COMMON_H
