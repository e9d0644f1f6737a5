"""rt_render_rays_async, GpuRenderer.render_rays and render_rays_into: what can be checked without a GPU.  The entry
point checks its arguments before any HIP call, so every refusal below happens on a machine without a device, and the
renderer checks shapes, dtypes, counts and modes before it touches its context."""
import ctypes
import re

import numpy as np
import pytest

from rt_mi355x import abi
from rt_mi355x import renderer as rmod
from test_abi import declared_functions
from test_query_abi import Dev, FakeDevice, NoGpu

HEADER = abi.SOURCE_FILES[-1]


def test_symbols_are_exported_and_declared():
    assert "rt_render_rays_async" in abi.EXPORTED and "rt_camera_rays" in abi.EXPORTED
    assert sorted(abi.EXPORTED) == declared_functions()
    text = open(HEADER).read()
    assert "int rt_render_rays_async(rt_context* ctx, uint64_t n_pixels, uint32_t spp, uint32_t rays_per_pixel," in text
    assert "int rt_camera_rays(const rt_projection* proj, uint32_t grid, uint32_t flags, void* origins, void* directions);" in text
    assert "rt_rays.hpp" in abi.KERNEL_SOURCES and "rt_projection.hpp" in abi.KERNEL_SOURCES
    src = abi.kernel_source_text()
    assert "trace_paths_rays" in src and "rays_validate" in src
    # the host ray generators stay free of HIP: the sanitizer program includes them alone
    proj = open([f for f in abi.SOURCE_FILES if f.endswith("rt_projection.hpp")][0]).read()
    assert "hip" not in proj.lower().replace("no hip", "")


def test_header_states_the_definition_and_what_is_out_of_scope():
    text = re.sub(r"\s*\n \*\s*", " ", open(HEADER).read())
    i = text.index("rendering caller-supplied primary rays")
    doc = text[i:text.index("int rt_render_rays_async(", i)]
    for phrase in ("1 <= R <= spp", "ray p R + (s mod R)", "directions are NOT normalised", "pix = pixel_base + p",
                   "Streams 0 and 1", "above 2^32 is RT_ERR_INVALID", "NaN x 3", "rgb8 is 0, 0, 0", "no RT_ERR_RANGE",
                   "the bounds included", "samples = valid pixels x spp", "RT_KERNEL_RAYS(kernel_id) is set",
                   "Out of scope: sample-parallel splitting, progressive sessions and guides over caller rays, the other "
                   "semantics modes, sorting or binning incoherent rays"):
        assert phrase in doc, phrase
    j = text.index("Host only, needs no GPU: the primary rays of three camera models")
    doc = text[j:text.index("int rt_camera_rays(", j)]
    for phrase in ("r = j grid + i", "((i + 0.5) / grid, (j + 0.5) / grid)", "rounded to T last",
                   "outside the image circle gets the direction 0, 0, 0", "renders that pixel black"):
        assert phrase in doc, phrase
    assert ctypes.sizeof(abi.RtProjection) == 3 * 4 + 4 + 11 * 8   # three words, padding, eleven doubles


def call(lib, ctx, n, spp, R, d_origins, origin, d_dirs, depth, base, flags, rgb, lin):
    o3 = None if origin is None else (ctypes.c_double * 3)(*origin)
    return lib.rt_render_rays_async(ctx, n, spp, R, d_origins, o3, d_dirs, depth, 1, base, flags, rgb, lin, None)


def test_arguments_are_refused_without_a_gpu(lib):
    p = ctypes.c_void_p(16)     # never dereferenced: the checks come first
    ctx = ctypes.c_void_p(16)
    O = (1.0, 2.0, 3.0)
    invalid = [
        ("NULL ctx", (None, 64, 4, 1, p, None, p, 8, 0, 0, p, p)),
        ("NULL directions", (ctx, 64, 4, 1, p, None, None, 8, 0, 0, p, p)),
        ("both origin forms", (ctx, 64, 4, 1, p, O, p, 8, 0, 0, p, p)),
        ("neither origin form", (ctx, 64, 4, 1, None, None, p, 8, 0, 0, p, p)),
        ("both outputs NULL", (ctx, 64, 4, 1, p, None, p, 8, 0, 0, None, None)),
        ("spp == 0", (ctx, 64, 0, 1, p, None, p, 8, 0, 0, p, p)),
        ("R == 0", (ctx, 64, 4, 0, p, None, p, 8, 0, 0, p, p)),
        ("R > spp", (ctx, 64, 4, 5, None, O, p, 8, 0, 0, p, None)),
        ("unknown flag bits", (ctx, 64, 4, 1, p, None, p, 8, 0, 0x20, p, p)),
        ("unknown flag bits with F32", (ctx, 64, 4, 4, None, O, p, 8, 0, abi.RT_FLAG_F32 | 0x100, None, p)),
        ("pixel_base + n_pixels above 2^32", (ctx, 64, 4, 1, p, None, p, 8, 0xFFFFFFC1, 0, p, p)),
    ]
    for what, args in invalid:
        assert call(lib, *args) == abi.RT_ERR_INVALID, what
        assert b"rt_render_rays_async" in lib.rt_last_error(), (what, lib.rt_last_error())
    for mode in (abi.RT_FLAG_MODE_VECTORIZED, abi.RT_FLAG_MODE_SCALAR, abi.RT_FLAG_MODE_VECTORIZED3,
                 abi.RT_FLAG_F32 | abi.RT_FLAG_ROOT2 | abi.RT_FLAG_MODE_SCALAR):
        assert call(lib, ctx, 64, 4, 1, p, None, p, 8, 0, mode, p, p) == abi.RT_ERR_UNSUPPORTED, mode
        assert b"rt_render_rays_async" in lib.rt_last_error()
    for flags in (0, abi.RT_FLAG_F32, abi.RT_FLAG_ROOT2, abi.RT_FLAG_F32 | abi.RT_FLAG_ROOT2):   # accepted flags
        assert call(lib, ctx, 0x80000000, 4, 1, p, None, p, 8, 0, flags, p, p) == abi.RT_ERR_UNSUPPORTED, flags
        assert b"too many pixels" in lib.rt_last_error()
        assert call(lib, ctx, 64, (1 << 20) + 1, 1, p, None, p, 8, 0, flags, p, p) == abi.RT_ERR_UNSUPPORTED
        assert b"spp > 2^20" in lib.rt_last_error()
    assert call(lib, ctx, 64, 4, 1, p, None, p, abi.RT_MAX_BOUNCES_F32 + 1, 0, abi.RT_FLAG_F32, p, p) == abi.RT_ERR_UNSUPPORTED
    assert b"RT_MAX_BOUNCES_F32" in lib.rt_last_error()
    # the last pixel a call may name is 2^32 - 1: it passes that check and stops at the next one (no scene: a context
    # that was never given one, here zeroed memory standing in for it, still before any HIP call)
    blank = ctypes.create_string_buffer(1 << 16)
    assert call(lib, blank, 64, 4, 1, p, None, p, 8, 0xFFFFFFC0, 0, p, p) == abi.RT_ERR_INVALID
    assert b"no scene set" in lib.rt_last_error()
    assert call(lib, blank, 0, 4, 1, p, None, p, 8, 0, 0, p, p) == abi.RT_ERR_INVALID   # before the n_pixels == 0 return
    assert b"no scene set" in lib.rt_last_error()


def test_kernel_rays_bit_decodes_alike_in_c_and_python():
    text = open(HEADER).read()
    m = re.search(r"#define RT_KERNEL_RAYS\(id\) \(\(\(id\) >> (\d+)\) & 1u\)", text)
    assert m and int(m.group(1)) == 13
    r = 0x8000 | 1 << 13
    for kid in (r | 6 << 1, r | 1 | 4 << 1 | 1 << 4 | 1 << 8, 0x808C, 0x8000 | 1 << 12, 0x8000 | 1 << 11 | 1 | 4 << 1):
        k = abi.kernel_info(kid)
        assert abi.RT_KERNEL_RAYS(kid) == (kid >> 13) & 1 and k["rays"] == bool(abi.RT_KERNEL_RAYS(kid))
    assert abi.kernel_name(r | 6 << 1) == "trace_paths_rays<float,6,false,false>"
    assert abi.kernel_name(r | 1 | 4 << 1 | 1 << 4 | 1 << 8) == "trace_paths_rays<double,4,true,true>"
    assert abi.kernel_name(0x808C) == "trace_paths<float,6,false,0,true,false>"   # existing names are unchanged
    assert abi.kernel_name(0x8000 | 1 << 12 | 1 | 4 << 1 | 1 << 7) == "query_rays<double,false,true,false>"


# ---------------------------------------------------------------- the renderer's own checks
D8 = np.zeros((8, 2, 3))


@pytest.mark.parametrize("flags", [abi.RT_FLAG_MODE_VECTORIZED, abi.RT_FLAG_MODE_SCALAR,
                                   abi.RT_FLAG_F32 | abi.RT_FLAG_MODE_VECTORIZED3])
def test_render_rays_refuses_modes_before_any_gpu_call(flags):
    with pytest.raises(ValueError, match="live path"):
        NoGpu(flags).render_rays(8, 4, np.zeros(3), D8, None)
    with pytest.raises(ValueError, match="live path"):
        NoGpu(flags).render_rays_into(8, 4, np.zeros(3), FakeDevice(D8), rgb=FakeDevice(np.zeros((8, 3), np.uint8)))


def test_render_rays_refuses_bad_arguments_before_any_gpu_call():
    r = NoGpu(abi.RT_FLAG_F32)
    for o, d in ((np.zeros(3), np.zeros((8, 2))), (np.zeros(3), np.zeros(8)), (np.zeros(3), np.zeros((2, 8, 3, 3))),
                 (np.zeros((8, 3)), D8), (np.zeros((8, 1, 3)), D8), (np.zeros(4), D8), (np.zeros((7, 2, 3)), D8)):
        with pytest.raises(ValueError, match="shape"):
            r.render_rays(8, 4, o, d, None)
    with pytest.raises(ValueError, match="numbers"):
        r.render_rays(8, 4, np.zeros(3), np.zeros((8, 3), dtype=complex), None)
    with pytest.raises(ValueError, match="rays per pixel"):
        r.render_rays(8, 1, np.zeros(3), D8, None)            # R = 2 > spp = 1
    for spp in (0, (1 << 20) + 1, 2.5, True):
        with pytest.raises(ValueError, match="spp"):
            r.render_rays(8, spp, np.zeros(3), D8, None)
    for base in (-1, (1 << 32) - 7, 1.5):
        with pytest.raises(ValueError, match="pixel_base"):
            r.render_rays(8, 4, np.zeros(3), D8, None, pixel_base=base)
    # what the checks hand on: (n, R, 3) in the renderer's precision, a shared origin kept in double
    o, d, shared = rmod.check_render_rays(abi.RT_FLAG_F32 | abi.RT_FLAG_ROOT2, 4, [1, 2, 3], np.zeros((8, 3)))
    assert shared and o.dtype == np.float64 and d.dtype == np.float32 and d.shape == (8, 1, 3) and d.flags.c_contiguous
    o, d, shared = rmod.check_render_rays(0, 4, np.zeros((8, 2, 3), np.float32), np.zeros((8, 2, 3), np.float32)[::-1],
                                          pixel_base=(1 << 32) - 8)
    assert not shared and o.dtype == d.dtype == np.float64 and o.shape == d.shape == (8, 2, 3) and d.flags.c_contiguous


def test_render_rays_into_refuses_bad_arrays_before_any_gpu_call():
    r = NoGpu(abi.RT_FLAG_F32, device=0)
    d = np.zeros((8, 2, 3), np.float32)
    rgb = FakeDevice(np.zeros((8, 3), np.uint8))
    with pytest.raises(TypeError, match="__cuda_array_interface__"):
        r.render_rays_into(8, 4, np.zeros(3), d, rgb=rgb)                       # a host array
    with pytest.raises(ValueError, match="dtype"):
        r.render_rays_into(8, 4, np.zeros(3), FakeDevice(np.zeros((8, 2, 3))), rgb=rgb)   # float64 in an fp32 renderer
    with pytest.raises(ValueError, match="shape"):
        r.render_rays_into(8, 4, np.zeros(3), FakeDevice(np.zeros((8, 2, 4), np.float32)), rgb=rgb)
    with pytest.raises(ValueError, match="shape"):
        r.render_rays_into(8, 4, FakeDevice(np.zeros((8, 3), np.float32)), FakeDevice(d), rgb=rgb)
    with pytest.raises(ValueError, match="origins"):
        r.render_rays_into(8, 4, np.zeros(2), FakeDevice(d), rgb=rgb)
    with pytest.raises(ValueError, match="contiguous"):
        r.render_rays_into(8, 4, np.zeros(3), FakeDevice(np.zeros((8, 2, 6), np.float32)[:, :, ::2]), rgb=rgb)
    with pytest.raises(ValueError, match="contiguous"):
        r.render_rays_into(8, 4, np.zeros(3), FakeDevice(d), rgb=FakeDevice(np.zeros((16, 3), np.uint8)[::2]))
    with pytest.raises(ValueError, match="dtype"):
        r.render_rays_into(8, 4, np.zeros(3), FakeDevice(d), rgb=FakeDevice(np.zeros((8, 3), np.int8)))
    with pytest.raises(ValueError, match="dtype"):
        r.render_rays_into(8, 4, np.zeros(3), FakeDevice(d), linear=FakeDevice(np.zeros((8, 3), np.float32)))
    with pytest.raises(ValueError, match="shape"):
        r.render_rays_into(8, 4, np.zeros(3), FakeDevice(d), linear=FakeDevice(np.zeros((8, 2, 3))))
    with pytest.raises(ValueError, match="read-only"):
        r.render_rays_into(8, 4, np.zeros(3), FakeDevice(d), rgb=FakeDevice(np.zeros((8, 3), np.uint8), readonly=True))
    with pytest.raises(ValueError, match="device"):
        r.render_rays_into(8, 4, np.zeros(3), FakeDevice(d, device=Dev("cuda", 1)), rgb=rgb)
    with pytest.raises(ValueError, match="device"):
        r.render_rays_into(8, 4, np.zeros(3), FakeDevice(d), linear=FakeDevice(np.zeros((8, 3)), device=Dev("cpu", None)))
    with pytest.raises(ValueError, match="no output"):
        r.render_rays_into(8, 4, np.zeros(3), FakeDevice(d))
    with pytest.raises(ValueError, match="rays per pixel"):
        r.render_rays_into(8, 1, np.zeros(3), FakeDevice(d), rgb=rgb)
    with pytest.raises(ValueError, match="pixel_base"):
        r.render_rays_into(8, 4, np.zeros(3), FakeDevice(d), rgb=rgb, pixel_base=1 << 32)
    with pytest.raises(TypeError, match="stream"):
        r.render_rays_into(8, 4, np.zeros(3), FakeDevice(d, device=Dev("cuda", 0)), rgb=rgb, stream="0")
    lin = FakeDevice(np.zeros((8, 3)))
    n, R, d_org, origin, d_dir, d_rgb, d_lin = rmod.check_render_rays_into(abi.RT_FLAG_F32, 0, 4, [1, 2, 3], FakeDevice(d),
                                                                           None, lin)
    assert (n, R) == (8, 2) and d_org is None and origin.dtype == np.float64 and d_dir == d.ctypes.data
    assert d_rgb is None and d_lin == lin.a.ctypes.data
    n, R, d_org, *_ = rmod.check_render_rays_into(0, 0, 1, FakeDevice(np.zeros((8, 3))), FakeDevice(np.zeros((8, 3))), rgb, None)
    assert (n, R) == (8, 1) and d_org
