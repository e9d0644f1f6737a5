"""A/B patch (round 11, rejected): nearest_hit's fp32 1 / a (objects.rs:254, a = |d|^2, once per sweep and lane)
without v_div_scale and v_div_fixup.  The compiler's correctly rounded division with numerator 1 is div_scale x2,
rcp, 6 FMAs, div_fmas, div_fixup; when every lane of the wave has 2^-126 <= a < 2^126 (a ballot) nothing is scaled
and nothing fixed, and rcp and the six FMAs alone give the same bits (1 x r1 is r1).  Checked on the device over every
bit pattern: all 2^23 x 252 arguments of the range, and their negatives, give the division's bits; from 2^126 up the
quotient is subnormal and the short form is wrong (tools/forms_probe.hip; profiles/r11/sqrt_forms.txt).  Otherwise the full division.
argv[2] = "if": the short form inside the ballot's branch; default: computed first, overwritten by the division
when the ballot finds a lane out of range.  Either shape costs the headline kernel two more SGPR spills."""
import sys
d = sys.argv[1]
shape = sys.argv[2] if len(sys.argv) > 2 else "overwrite"
p = f"{d}/rt_device.hpp"
s = open(p).read()
anchor = "template <typename T> __device__ __forceinline__ V3<T> neg(V3<T> a)"
assert s.count(anchor) == 1
body = {"overwrite": """    const float r0 = __builtin_amdgcn_rcpf(a);
    const float r1 = __builtin_fmaf(__builtin_fmaf(-a, r0, 1.0f), r0, r0);
    const float f3 = __builtin_fmaf(__builtin_fmaf(-a, r1, 1.0f), r1, r1);
    float q = __builtin_fmaf(__builtin_fmaf(-a, f3, 1.0f), r1, f3);
    if (__builtin_expect(__ballot(!(a >= 0x1.0p-126f && a < 0x1.0p126f)) != 0ull, 0)) q = 1.0f / a;
    return q;
""", "if": """    if (__builtin_expect(__ballot(!(a >= 0x1.0p-126f && a < 0x1.0p126f)) == 0ull, 1)) {
        const float r0 = __builtin_amdgcn_rcpf(a);
        const float r1 = __builtin_fmaf(__builtin_fmaf(-a, r0, 1.0f), r0, r0);
        const float f3 = __builtin_fmaf(__builtin_fmaf(-a, r1, 1.0f), r1, r1);
        return __builtin_fmaf(__builtin_fmaf(-a, f3, 1.0f), r1, f3);
    }
    return 1.0f / a;
"""}[shape]
s = s.replace(anchor, "__device__ __forceinline__ float rcp_len(float a) {\n" + body + "}\n"
              "__device__ __forceinline__ double rcp_len(double a) { return 1.0 / a; }\n" + anchor)
open(p, "w").write(s)
p = f"{d}/rt_sweep.hpp"
s = open(p).read()
old = "const T inv_a = SCALAR ? T(0) : T(1.0) / a;      // objects.rs:254 (loop-invariant)"
assert s.count(old) == 1
s = s.replace(old, "const T inv_a = SCALAR ? T(0) : rcp_len(a);      // objects.rs:254 (loop-invariant)")
open(p, "w").write(s)
