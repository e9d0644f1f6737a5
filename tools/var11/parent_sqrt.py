"""A/B patch (round 11), applied to the product sources: sqrt_nd and sqrt_len as the parent commit had them
(v_sqrt_f32 and the two-neighbour correction; sqrt_len's ballot on tiny nonzero arguments only), so the variant
is the product without the rsq form: rcp_len alone."""
import re
import sys
d = sys.argv[1]
p = f"{d}/rt_device.hpp"
s = open(p).read()
nd = re.search(r"__device__ __forceinline__ float sqrt_nd\(float x\) \{.*?\n\}", s, re.S)
ln = re.search(r"__device__ __forceinline__ float sqrt_len\(float x\) \{.*?\n\}", s, re.S)
assert nd and ln and "sqrt_rg" in nd.group(0) and "sqrt_rg" in ln.group(0)
s = s.replace(nd.group(0), """__device__ __forceinline__ float sqrt_nd(float x) {
    const float s = __builtin_amdgcn_sqrtf(x);
    const float sdn = __int_as_float(__float_as_int(s) - 1), sup = __int_as_float(__float_as_int(s) + 1);
    float r = __builtin_fmaf(-sdn, s, x) <= 0.0f ? sdn : s;
    r = __builtin_fmaf(-sup, s, x) > 0.0f ? sup : r;
    return r;
}""")
s = s.replace(ln.group(0), """__device__ __forceinline__ float sqrt_len(float x) {
    if (__builtin_expect(__ballot(x != 0.0f && fabsf(x) < 0x1.0p-96f) == 0ull, 1)) return sqrt_nd(x);
    return sqrtf(x);
}""")
open(p, "w").write(s)
