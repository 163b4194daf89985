"""The BZip2 reader's entry points in the ASan + UBSan build of the product's host side (`make asan`, as test_host_asan.py): their argument checks
come before anything touches a device, so they are driven here without one -- no context, and, where a device lets a context be made, null
buffers, negative counts and sizes of 1 TiB and more."""
import glob
import os
import subprocess
import sys

from _common import ROOT

DRIVER = r'''
import ctypes, os
ROOT = %(root)r
L = ctypes.CDLL(os.path.join(ROOT, "zip-ada_amd", "variants", "libzada_hip_asan.so"))
vp, u64, i32, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint32
L.zada_create.restype = vp; L.zada_create.argtypes = [i32]
L.zada_destroy.argtypes = [vp]
L.zada_last_error.restype = ctypes.c_char_p; L.zada_last_error.argtypes = [vp]
L.zada_bunzip2.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp]
L.zada_bunzip2_device.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp]
L.zada_bunzip2_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
L.zada_bunzip2_last_records.restype = u64; L.zada_bunzip2_last_records.argtypes = [vp, i32, vp, u64]
L.zada_set_knob.argtypes = [vp, ctypes.c_char_p, i32]
buf = ctypes.create_string_buffer(4096)
b = ctypes.cast(buf, vp)
ol, iu, reg = u64(77), u64(77), u32(0x1234)
refs = (ctypes.byref(ol), ctypes.byref(iu), ctypes.byref(reg))
E_INVALID, E_TOO_LARGE = -1, -4
# no context: ZADA_E_INVALID (or no items), nothing touched
for f in (L.zada_bunzip2, L.zada_bunzip2_device):
    assert f(None, b, 64, b, 64, *refs) == E_INVALID and f(None, None, 0, None, 0, None, None, None) == E_INVALID
assert L.zada_bunzip2_batch(None, 1, b, b, b, b, b, b, b, b) == E_INVALID and L.zada_bunzip2_batch(None, 0, None, None, None, None, None, None, None, None) == E_INVALID
assert L.zada_bunzip2_last_records(None, 0, b, 8) == 0 and L.zada_bunzip2_last_records(None, 1, None, 0) == 0
assert (ol.value, iu.value, reg.value) == (77, 77, 0x1234)
assert L.zada_set_knob(None, b"bunzip_batch_mib", 64) == E_INVALID
ctx = L.zada_create(0)
if ctx:                                              # a box with a GPU: the checks that stand before the first device call
    assert L.zada_set_knob(ctx, b"bunzip_batch_mib", 0) == E_INVALID and L.zada_set_knob(ctx, b"bunzip_batch_mib", 64) == 0
    for f, who in ((L.zada_bunzip2, b"zada_bunzip2"), (L.zada_bunzip2_device, b"zada_bunzip2_device")):
        assert f(ctx, None, 5, b, 64, *refs) == E_INVALID and who in L.zada_last_error(ctx)
        assert f(ctx, b, 5, None, 64, *refs) == E_INVALID
    assert L.zada_bunzip2_device(ctx, b, 1 << 40, b, 64, *refs) == E_TOO_LARGE and L.zada_bunzip2_device(ctx, b, 64, b, (1 << 64) - 8, *refs) == E_TOO_LARGE
    ptrs = (u64 * 2)(b.value, 0); lens = (u64 * 2)(64, 64); caps = (u64 * 2)(64, 1 << 40); rcs = (i32 * 2)(9, 9)
    assert L.zada_bunzip2_batch(ctx, -1, ptrs, lens, ptrs, caps, None, None, None, rcs) == E_INVALID
    assert L.zada_bunzip2_batch(ctx, 2, ptrs, lens, None, caps, None, None, None, None) == E_INVALID            # no rc array
    assert L.zada_bunzip2_batch(ctx, 2, ptrs, lens, None, caps, None, None, None, rcs) == E_INVALID             # a null stream of 64 bytes
    ptrs[1] = b.value
    assert L.zada_bunzip2_batch(ctx, 2, ptrs, lens, None, caps, None, None, None, rcs) == E_TOO_LARGE and tuple(rcs) == (9, 9)
    assert L.zada_bunzip2_batch(ctx, 0, None, None, None, None, None, None, None, None) == 0
    assert L.zada_bunzip2_last_records(ctx, 0, None, 5) == 0
    assert (ol.value, iu.value, reg.value) == (77, 77, 0x1234)
    L.zada_destroy(ctx)
print("bunzip2 host asan ok", bool(ctx))
'''


def test_bunzip2_argument_checks_are_clean_under_asan_and_ubsan():
    lib = os.path.join(ROOT, "zip-ada_amd", "variants", "libzada_hip_asan.so")
    srcs = glob.glob(os.path.join(ROOT, "zip-ada_amd", "csrc", "*.h*")) + [os.path.join(ROOT, "include", "zada.h")]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(p) for p in srcs):      # (test_host_asan.py builds it too: once is enough)
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "zip-ada_amd", "csrc"), "asan"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    rt = glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.so")
    assert rt, "clang's ASan runtime (hipcc's) is not installed"
    env = dict(os.environ, LD_PRELOAD=" ".join(x for x in (rt[0], os.environ.get("LD_PRELOAD", "")) if x), ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:protect_shadow_gap=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([sys.executable, "-c", DRIVER % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "bunzip2 host asan ok" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
