"""A/B patch (round 11), applied to the product sources: sqrt_rg's 1/2 held in a VGPR (an opaque v_mov_b32, which the
compiler may hoist and share) instead of an inline constant, so that h = g / 2 is an all-VGPR multiply and can
co-issue (tools/issue_weights.json: 2.6 SIMD-cycles against 4.7 with a constant operand)."""
import sys
d = sys.argv[1]
p = f"{d}/rt_device.hpp"
s = open(p).read()
old = "    const float s = x * g, h = 0.5f * g;\n"
assert s.count(old) == 1
s = s.replace(old, """    float half;
    asm("v_mov_b32 %0, 0.5" : "=v"(half));
    const float s = x * g, h = half * g;
""")
open(p, "w").write(s)
