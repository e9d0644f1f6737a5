// Round-11 probe (profiles/r11/sqrt_forms.txt): candidate short forms of the fp32 square root over every bit pattern
// of [2^-96, +inf) against sqrtf, and of 1 / a (tools/var11/rcp_len.py) over every normal a against 1.0f / a, per
// biased exponent; the library results are the correctly rounded ones of the same build.  One launch, under a second.
//   hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -std=c++17 -o tools/bin/forms_probe tools/forms_probe.hip
// Form B-short is the product's sqrt_rg (rt_device.hpp), which tests/test_gpu_sqrt_forms.py checks on its own.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#define NC 6
struct Out {
    unsigned long long bad[NC];
    uint32_t first[NC][8];
    unsigned long long inv_bad_exp[256];   // reciprocal form: mismatches per biased exponent of a
    unsigned long long inv_n_exp[256];
};

__device__ __forceinline__ float sq_b(float x) {   // rsq + coupled Goldschmidt step + residual
    const float g = __builtin_amdgcn_rsqf(x);
    float s = x * g, h = 0.5f * g;
    const float e = __builtin_fmaf(-h, s, 0.5f);
    h = __builtin_fmaf(h, e, h);
    s = __builtin_fmaf(s, e, s);
    const float d = __builtin_fmaf(-s, s, x);
    return __builtin_fmaf(d, h, s);
}
__device__ __forceinline__ float sq_bshort(float x) {   // rsq + residual only
    const float g = __builtin_amdgcn_rsqf(x);
    const float s = x * g, h = 0.5f * g;
    const float d = __builtin_fmaf(-s, s, x);
    return __builtin_fmaf(d, h, s);
}
__device__ __forceinline__ float sq_c(float x) {   // sqrt + rsq, one residual
    const float s = __builtin_amdgcn_sqrtf(x);
    const float h = 0.5f * __builtin_amdgcn_rsqf(x);
    const float d = __builtin_fmaf(-s, s, x);
    return __builtin_fmaf(d, h, s);
}
__device__ __forceinline__ float sq_d(float x) {   // sqrt, h = 0.5 * rcp(s), one residual
    const float s = __builtin_amdgcn_sqrtf(x);
    const float h = 0.5f * __builtin_amdgcn_rcpf(s);
    const float d = __builtin_fmaf(-s, s, x);
    return __builtin_fmaf(d, h, s);
}
__device__ __forceinline__ float sq_e(float x) {   // B with the residual step from the unrefined h
    const float g = __builtin_amdgcn_rsqf(x);
    float s = x * g;
    const float h = 0.5f * g;
    const float e = __builtin_fmaf(-h, s, 0.5f);
    s = __builtin_fmaf(s, e, s);
    const float d = __builtin_fmaf(-s, s, x);
    return __builtin_fmaf(d, h, s);
}
__device__ __forceinline__ float sq_f(float x) {   // B-short with the residual step as an unfused multiply and add
    const float g = __builtin_amdgcn_rsqf(x);
    const float s = x * g, h = 0.5f * g;
    return s + __builtin_fmaf(-s, s, x) * h;
}
__device__ __forceinline__ float inv_fast(float a) {
    const float r0 = __builtin_amdgcn_rcpf(a);
    const float r1 = __builtin_fmaf(__builtin_fmaf(-a, r0, 1.0f), r0, r0);
    const float f3 = __builtin_fmaf(__builtin_fmaf(-a, r1, 1.0f), r1, r1);
    return __builtin_fmaf(__builtin_fmaf(-a, f3, 1.0f), r1, f3);
}
__device__ __forceinline__ bool same(float a, float b) {
    return (a != a && b != b) || __float_as_uint(a) == __float_as_uint(b);
}

__global__ void probe(Out* o) {
    __shared__ unsigned long long sb[256], sn[256];
    for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) { sb[i] = 0; sn[i] = 0; }
    __syncthreads();
    const uint64_t n = 1ull << 32, stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < n; b += stride) {
        const uint32_t u = (uint32_t)b;
        const float x = __uint_as_float(u);
        if (x >= 0x1.0p-96f && x < __builtin_inff()) {
            const float ref = sqrtf(x);
            const float c[NC] = {sq_b(x), sq_bshort(x), sq_c(x), sq_d(x), sq_e(x), sq_f(x)};
#pragma unroll
            for (int k = 0; k < NC; ++k)
                if (!same(c[k], ref)) {
                    const unsigned long long slot = atomicAdd(&o->bad[k], 1ull);
                    if (slot < 8) o->first[k][slot] = u;
                }
        }
        const uint32_t ex = (u >> 23) & 255u;
        if (ex != 0u && ex != 255u) {
            const float ref = 1.0f / x;
            atomicAdd(&sn[ex], 1ull);
            if (!same(inv_fast(x), ref)) atomicAdd(&sb[ex], 1ull);
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) {
        if (sb[i]) atomicAdd(&o->inv_bad_exp[i], sb[i]);
        if (sn[i]) atomicAdd(&o->inv_n_exp[i], sn[i]);
    }
}

int main() {
    Out* d;
    if (hipMalloc(&d, sizeof(Out)) != hipSuccess) return 2;
    if (hipMemset(d, 0, sizeof(Out)) != hipSuccess) return 2;
    probe<<<2048, 256>>>(d);
    if (hipDeviceSynchronize() != hipSuccess) { printf("kernel failed\n"); return 3; }
    Out h;
    if (hipMemcpy(&h, d, sizeof(Out), hipMemcpyDeviceToHost) != hipSuccess) return 2;
    const char* nm[NC] = {"B rsq+goldschmidt+residual", "B-short rsq+residual", "C sqrt+rsq residual", "D sqrt+rcp residual",
                          "E rsq+half step+residual(h0)", "F B-short, residual unfused"};
    for (int k = 0; k < NC; ++k) {
        printf("%-32s mismatches %llu first:", nm[k], h.bad[k]);
        for (int j = 0; j < 8 && (unsigned long long)j < h.bad[k]; ++j) printf(" %08x", h.first[k][j]);
        printf("\n");
    }
    printf("inv_fast mismatches per biased exponent (nonzero only), of 2^24 each:\n");
    for (int e = 1; e < 255; ++e)
        if (h.inv_bad_exp[e]) printf("  exp %d (2^%d): %llu / %llu\n", e, e - 127, h.inv_bad_exp[e], h.inv_n_exp[e]);
    printf("done\n");
    return 0;
}
