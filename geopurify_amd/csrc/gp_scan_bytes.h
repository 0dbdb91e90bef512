// Temporary storage of a rocPRIM exclusive plus-scan over n elements of T (the size query: nothing is launched).
#pragma once
#include <rocprim/device/device_scan.hpp>
#include <stddef.h>
#include <stdint.h>

template <typename T>
inline size_t gp_scan_bytes(int64_t n) {
    size_t t = 0;
    (void)rocprim::exclusive_scan(nullptr, t, (T *)nullptr, (T *)nullptr, (T)0, (size_t)n, rocprim::plus<T>(), 0);
    return t;
}
