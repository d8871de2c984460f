// Selection builders of the FILTERED search (acamd.h "FILTERED search"): a device bitmap of 64-bit words, row r = bit r % 64 of
// word r / 64, bit 0 the least significant -- byte for byte faiss's IDSelectorBitmap layout on this little-endian target.
//
//  knn_sel_pack_kernel     bit r = (mask[r] != 0)                                      (a bool / uint8 mask)
//  knn_sel_classes_kernel  bit r = class_on[row_class[r]] != 0, a class outside [0, n_classes) gives 0   (an int32 row -> class map)
//
// One lane tests one row, a wave ballot IS the word, lane 0 of the wave stores it: every word of ceil(n / 64) has exactly one
// writer, the lanes past n vote 0 (so the tail bits of the last word are written as 0), nothing past the last word is touched,
// no atomics, no host synchronisation.
#include "common.h"

namespace {

constexpr int kSelThreads = 256;       // 4 waves = 4 words per workgroup

template <typename Test>
__device__ __forceinline__ void sel_ballot_store(int64_t n, uint64_t* sel, Test test) {
    const int64_t r = (int64_t)blockIdx.x * kSelThreads + threadIdx.x;
    const bool on = r < n && test(r);
    const unsigned long long word = __builtin_amdgcn_ballot_w64(on);
    const int64_t w = r >> 6;                                           // (wave-uniform: a wave covers rows 64 w .. 64 w + 63)
    if ((threadIdx.x & 63) == 0 && 64 * w < n) sel[w] = (uint64_t)word;
}

__global__ __launch_bounds__(kSelThreads) void knn_sel_pack_kernel(const uint8_t* mask, int64_t n, uint64_t* sel) {
    sel_ballot_store(n, sel, [&](int64_t r) { return mask[r] != 0; });
}

__global__ __launch_bounds__(kSelThreads) void knn_sel_classes_kernel(const int32_t* row_class, int64_t n, const uint8_t* class_on,
                                                                      int n_classes, uint64_t* sel) {
    sel_ballot_store(n, sel, [&](int64_t r) {
        const int32_t c = row_class[r];
        return c >= 0 && c < n_classes && class_on[c] != 0;
    });
}

}  // namespace

extern "C" int ac_knn_sel_pack(const uint8_t* d_mask, int64_t n, uint64_t* d_sel, ac_stream_t stream_) {
    AC_REQUIRE(n >= 0 && n < 2147483647LL * 64, AC_EINVAL, "knn_sel_pack: n=%lld out of range", (long long)n);
    if (n == 0) return AC_OK;
    AC_REQUIRE(d_mask != nullptr, AC_EINVAL, "knn_sel_pack: d_mask is NULL");
    AC_REQUIRE(d_sel != nullptr && (((uintptr_t)d_sel) & 7) == 0, AC_EINVAL, "knn_sel_pack: d_sel must be non-NULL and 8-byte aligned");
    hipLaunchKernelGGL(knn_sel_pack_kernel, dim3((unsigned)((n + kSelThreads - 1) / kSelThreads)), dim3(kSelThreads), 0,
                       (hipStream_t)stream_, d_mask, n, d_sel);
    AC_LAUNCH_CHECK();
    return AC_OK;
}

extern "C" int ac_knn_sel_classes(const int32_t* d_row_class, int64_t n, const uint8_t* d_class_on, int n_classes, uint64_t* d_sel,
                                  ac_stream_t stream_) {
    AC_REQUIRE(n >= 0 && n < 2147483647LL * 64, AC_EINVAL, "knn_sel_classes: n=%lld out of range", (long long)n);
    AC_REQUIRE(n_classes >= 0, AC_EINVAL, "knn_sel_classes: n_classes=%d must be >= 0", n_classes);
    if (n == 0) return AC_OK;
    AC_REQUIRE(d_row_class != nullptr && (d_class_on != nullptr || n_classes == 0), AC_EINVAL, "knn_sel_classes: d_row_class / d_class_on is NULL");
    AC_REQUIRE(d_sel != nullptr && (((uintptr_t)d_sel) & 7) == 0, AC_EINVAL, "knn_sel_classes: d_sel must be non-NULL and 8-byte aligned");
    hipLaunchKernelGGL(knn_sel_classes_kernel, dim3((unsigned)((n + kSelThreads - 1) / kSelThreads)), dim3(kSelThreads), 0,
                       (hipStream_t)stream_, d_row_class, n, d_class_on, n_classes, d_sel);
    AC_LAUNCH_CHECK();
    return AC_OK;
}
