// rt_devforms.hip — TEST INFRASTRUCTURE ONLY: the fp32 short forms of csrc/rt_device.hpp (sqrt_rg, sqrt_nd,
// sqrt_len) against the correctly rounded library sqrtf of the same build, compared on the device
// (tests/devforms_bind.py, tests/test_gpu_sqrt_forms.py).  Built with rt_devunit.hip into
// lib/librt_devunit.so; the product library never links it and it is not part of the source hash.
//
// The sweep runs every one of the 2^32 bit patterns in one launch, 64 consecutive patterns to a wave, and returns
// the number of results that differ from the library's (two NaNs are equal) and the first eight offending inputs.
// The map kernel takes whole waves the caller arranged (n a multiple of 256, no early return), so the wave ballot
// inside sqrt_len sees the caller's lanes only; it returns the form's bits and the library's side by side.
#include "rt_device.hpp"
#include <initializer_list>

using namespace rt;

namespace {

constexpr unsigned kBlock = 256;
constexpr unsigned kGrid = 1u << 14;
constexpr uint32_t kIters = (uint32_t)((1ull << 32) / kBlock / kGrid);
constexpr uint32_t kFirst = 8;

__device__ __forceinline__ bool same_bits(float a, float b) {
    return (a != a && b != b) || __float_as_uint(a) == __float_as_uint(b);
}
__device__ __forceinline__ void report(uint32_t bits, unsigned long long* count, uint32_t* first) {
    const unsigned long long slot = atomicAdd(count, 1ull);
    if (slot < kFirst) first[slot] = bits;
}

// which 0: sqrt_nd on +-0, |x| >= 2^-96, +-inf, NaN (its documented domain and -inf); 1: sqrt_rg on [2^-96, +inf).
// A pattern outside the form's domain is counted in count[1] and not tested.
__global__ void k_sqrt_forms(int which, unsigned long long* count, uint32_t* first) {
#pragma unroll 1
    for (uint32_t it = 0; it < kIters; ++it) {
        const uint32_t bits = (it * kGrid + blockIdx.x) * kBlock + threadIdx.x;
        const float x = __uint_as_float(bits);
        const bool in = which == 0 ? !(x != 0.0f && fabsf(x) < 0x1.0p-96f) : (x >= 0x1.0p-96f && x < __builtin_inff());
        const unsigned long long out = __ballot(!in);   // every lane of the wave is here
        if (out != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(count + 1, (unsigned long long)__popcll(out));
        if (!in) continue;
        const float got = which == 0 ? sqrt_nd(x) : sqrt_rg(x);
        if (!same_bits(got, sqrtf(x))) report(bits, count, first);
    }
}

__global__ void k_sqrt_len_map(const float* x, float* got, float* want, size_t) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    got[i] = sqrt_len(x[i]);
    want[i] = sqrtf(x[i]);
}

struct Buf {
    void* p = nullptr;
    hipError_t err;
    explicit Buf(size_t bytes) { err = hipMalloc(&p, bytes ? bytes : 1); }
    ~Buf() { if (p) (void)hipFree(p); }
};
hipError_t first_err(std::initializer_list<hipError_t> es) {
    for (hipError_t e : es) if (e != hipSuccess) return e;
    return hipSuccess;
}

// count[2] (mismatches, patterns skipped), first[8]
template <typename K> int sweep(K&& launch, uint64_t* mismatches, uint64_t* skipped, uint32_t* first) {
    Buf c(2 * sizeof(unsigned long long)), f(kFirst * sizeof(uint32_t));
    hipError_t e = first_err({c.err, f.err});
    if (e == hipSuccess) e = first_err({hipMemset(c.p, 0, 2 * sizeof(unsigned long long)), hipMemset(f.p, 0, kFirst * sizeof(uint32_t))});
    if (e != hipSuccess) return (int)e;
    launch((unsigned long long*)c.p, (uint32_t*)f.p);
    unsigned long long h[2] = {0, 0};
    e = first_err({hipGetLastError(), hipDeviceSynchronize(), hipMemcpy(h, c.p, sizeof h, hipMemcpyDeviceToHost),
                   hipMemcpy(first, f.p, kFirst * sizeof(uint32_t), hipMemcpyDeviceToHost)});
    *mismatches = h[0];
    *skipped = h[1];
    return (int)e;
}

template <typename K> int map2(K kern, const float* x, float* got, float* want, size_t n) {
    if (n == 0 || n % kBlock != 0) return -1;
    Buf dx(n * sizeof(float)), dg(n * sizeof(float)), dw(n * sizeof(float));
    hipError_t e = first_err({dx.err, dg.err, dw.err});
    if (e == hipSuccess) e = hipMemcpy(dx.p, x, n * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kern, dim3((unsigned)(n / kBlock)), dim3(kBlock), 0, 0, (const float*)dx.p, (float*)dg.p, (float*)dw.p, n);
    e = first_err({hipGetLastError(), hipDeviceSynchronize(), hipMemcpy(got, dg.p, n * sizeof(float), hipMemcpyDeviceToHost),
                   hipMemcpy(want, dw.p, n * sizeof(float), hipMemcpyDeviceToHost)});
    return (int)e;
}

}  // namespace

extern "C" {

int du_sqrt_forms_sweep(int which, uint64_t* mismatches, uint64_t* skipped, uint32_t* first) {
    if (which < 0 || which > 1) return -1;
    return sweep([&](unsigned long long* c, uint32_t* f) { hipLaunchKernelGGL(k_sqrt_forms, dim3(kGrid), dim3(kBlock), 0, 0, which, c, f); },
                 mismatches, skipped, first);
}
int du_sqrt_len_map(const float* x, float* got, float* want, size_t n) { return map2(k_sqrt_len_map, x, got, want, n); }

}  // extern "C"
