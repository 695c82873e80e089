"""The post-processing kernels (csrc/pt_post.h: pt_post_pfm_kernel, pt_post_loglum_kernel + pt_post_sum_kernel,
pt_post_tonemap_kernel) at frame sizes, in fp32 and fp64, staged and resident, against tests/post_reference.py -- a plain numpy
/ fsum / mpmath restatement that tests/test_postprocess.py pins to the oracle and to the g10 goldens on the CPU.

Inputs come from fixed seeds.  Every size is chosen from a constant of the code (post_reference.POST_CHUNK = 8192 pixels per
luminosity block; post_grid(): 4096 blocks x 256 threads = 1 048 576 threads per grid-stride trip):

  1x1, 1x2, 3x1             degenerate
  8191x1, 8192x1, 8193x1    one short of / exactly / one past a luminosity chunk
  349525x1, 349526x1        W*3 = 1 048 575 / 1 048 578: the last value of the first trip / the first values of the second
  1279x719                  odd, 2.76 M values: three trips
  2049x1024                 257 partials: the second-level sum's first loop
  3840x2160                 1013 partials, 24 trips
  1x100003                  one-pixel rows: the PFM flip with rem < 3 always

What must be exact is asserted exact: PFM bytes, the tone-mapped image for a given scale (IEEE multiply and divide, no
contraction), LDR bytes at gamma 1.0.  What goes through log10 / pow is bounded from the measured distance of the device's
functions to the exact ones (L_LOG10, P_POW below; test_device_log10_and_pow_distance prints what it sees)."""
import ctypes as C
import functools
import io
import math

import numpy as np
import pytest

from pytracer_amd import _lib, abi

from . import post_reference as R

pytestmark = pytest.mark.gpu

# Distance of the device's log10 and pow to the exact value, measured on an MI355X over the domains used here (log10 on
# 1e-10 .. 1e4; pow(x, 1/2.2) on [0, 1) and 1e-6 .. 1e4; pow(10, y) on -10 .. 4; 200 000 values each against extended
# precision, the first 5000 of each against mpmath at 50 digits; profiles/CHANGELOG.md has the figures).
# Each constant is twice the observed maximum rounded up to a whole unit: the factor of two is for inputs the sample missed.
L_LOG10 = 3.0   # in units of U * |t| (an ulp is between one and two of those).  Observed: 1.127 U|t| (0.618 ulp)
P_POW = 3.0     # ulp.  Observed: 1.301 ulp for pow(x, 1/2.2), 1.333 ulp for pow(10, y)
K_LDR = P_POW + 1  # a product within K ulp of an integer may truncate to either side (post_reference.ldr_bytes)
# libm's pow(10, .) on the host -- pt_image_average_luminosity ends in std::pow, the reference in Python's 10 ** y, the same
# function: below 1 ulp by glibc's own claim, checked against mpmath in tests/test_postprocess.py
P_HOST = 1.0

PT_ERR_INVALID = -1  # include/ptrace.h

SIZES = [(1, 1), (1, 2), (3, 1),
         (R.POST_CHUNK - 1, 1), (R.POST_CHUNK, 1), (R.POST_CHUNK + 1, 1),
         (R.GRID_THREADS // 3, 1), (R.GRID_THREADS // 3 + 1, 1),
         (1279, 719), (2049, 1024), (3840, 2160), (1, 100003)]
assert R.GRID_THREADS // 3 * 3 == R.GRID_THREADS - 1 and -(-2049 * 1024 // R.POST_CHUNK) == R.POST_THREADS + 1
DTYPES = [np.float64, np.float32]
_ids = dict(ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else getattr(v, "__name__", str(v)))


@pytest.fixture(scope="module", autouse=True)
def dev():
    from pytracer_amd import device

    if device.device_count() < 1:
        pytest.skip("no HIP device")
    return device


# ---- inputs ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=3)
def _image(kind, W, H, dtype):
    """(a) 'uniform': [0, 1).  (b) 'hdr': log-uniform over 1e-6 .. 1e4, a quarter of the pixels exactly black.
    'positive': (a) without zeros, for delta = 0."""
    rng = np.random.default_rng([W, H, {"uniform": 1, "hdr": 2, "positive": 3}[kind]])
    if kind == "hdr":
        img = 10.0 ** rng.uniform(-6.0, 4.0, (H, W, 3))
        img[rng.random((H, W)) < 0.25] = 0.0
    else:
        img = rng.random((H, W, 3))
        if kind == "positive":
            img = img + 2.0 ** -10
    img = img.astype(dtype)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=1)
def _hip_runtime():
    """The HIP runtime this process already holds (libptrace.so brought it in): hipMemcpy, to fill a DeviceBuffer."""
    _lib.lib()
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64.so" in line}
    assert len(paths) == 1, paths
    hip = C.CDLL(paths.pop())
    hip.hipMemcpy.restype = C.c_int
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


def _legs(arr):
    """-> [(name, make)]: make() -> a fresh DeviceImage holding a copy of `arr` as a host array (staged by the C-ABI), in a
    devmem.DeviceBuffer, and in a CUDA torch tensor (left out when torch sees no device)."""
    from pytracer_amd.devmem import DeviceBuffer
    from pytracer_amd.postprocess import DeviceImage

    def host():
        return DeviceImage(arr.copy())

    def buffer():
        buf = DeviceBuffer(arr.shape, arr.dtype)
        assert _hip_runtime().hipMemcpy(buf.data_ptr(), arr.ctypes.data, arr.nbytes, 1) == 0  # hipMemcpyHostToDevice
        return DeviceImage(buf)

    legs = [("host", host), ("buffer", buffer)]
    try:
        import torch

        if torch.cuda.is_available():
            legs.append(("torch", lambda: DeviceImage(torch.from_numpy(arr.copy()).cuda())))
    except ImportError:
        pass
    return legs


def _same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the functions themselves -----------------------------------------------------------------------------------------------
def test_device_log10_and_pow_distance(dev):
    """L_LOG10 and P_POW hold on this device, and by how much (ops 12 and 13 of the probe kernel)."""
    rng = np.random.default_rng(11)
    n = 200_000
    x = 10.0 ** rng.uniform(-10.0, 4.0, n)
    got = dev.probe(12, x)
    ulp, units = R.distance(got, np.log10(x.astype(np.longdouble)))
    print(f"log10 on 1e-10..1e4: {ulp:.3f} ulp, {units:.3f} U|t| (L_LOG10 = {L_LOG10})")
    assert units <= L_LOG10
    # ... and against the reference's own terms, which is what the luminosity bound is about
    assert R.distance(got, np.log10(x.astype(np.longdouble)).astype(np.float64))[1] <= L_LOG10
    inv = 1.0 / 2.2
    worst = 0.0
    for name, a, b in (("pow(x, 1/2.2) on [0, 1)", rng.random(n), np.full(n, inv)),
                       ("pow(x, 1/2.2) on 1e-6..1e4", 10.0 ** rng.uniform(-6.0, 4.0, n), np.full(n, inv)),
                       ("pow(10, y) on -10..4", np.full(n, 10.0), rng.uniform(-10.0, 4.0, n))):
        got = dev.probe(13, a, b)
        ulp, _ = R.distance(got, np.power(a.astype(np.longdouble), b.astype(np.longdouble)))
        print(f"{name}: {ulp:.3f} ulp (P_POW = {P_POW})")
        worst = max(worst, ulp)
        if R.mpmath is not None:  # the extended-precision figures against 50 digits, on a sample
            ulp_mp, _ = R.exact_distance("pow", got[:5000], a[:5000], b[:5000])
            print(f"  ... first 5000 against mpmath: {ulp_mp:.3f} ulp")
            worst = max(worst, ulp_mp)
    assert worst <= P_POW
    if R.mpmath is not None:
        ulp_mp, units_mp = R.exact_distance("log10", dev.probe(12, x[:5000]), x[:5000])
        print(f"log10, first 5000 against mpmath: {ulp_mp:.3f} ulp, {units_mp:.3f} U|t|")
        assert units_mp <= L_LOG10
    # ocml's pow(x, 1.0) is not always x: within P_POW like any other power, which is why the tone-map
    # kernel does not call it at gamma 1.0 (test_ldr_bytes_on_the_truncation_steps)
    k = np.arange(256) / 255
    x1 = np.concatenate([rng.random(n), 10.0 ** rng.uniform(-6.0, 4.0, n), k, np.nextafter(k, -1.0), np.nextafter(k, 2.0)])
    got = dev.probe(13, x1, np.ones_like(x1))
    ulp, _ = R.distance(got, x1)
    print(f"pow(x, 1.0) != x for {int((got != x1).sum())} of {x1.size} values, at most {ulp:.3f} ulp away")
    assert ulp <= P_POW


# ---- PFM ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("size", SIZES, **_ids)
def test_pfm_payload_is_byte_exact(size, dtype):
    W, H = size
    arr = _image("hdr", W, H, dtype)
    want = {be: R.pfm_payload(arr, be) for be in (False, True)}
    for name, make in _legs(arr):
        img = make()
        for be in (False, True):
            got = img.pfm_payload(2 if be else 1)
            assert len(got) == W * H * 12
            if got != want[be]:
                first = int(np.argmax(np.frombuffer(got, dtype=np.uint8) != np.frombuffer(want[be], dtype=np.uint8)))
                pytest.fail(f"{name}, {'big' if be else 'little'} endian: first difference at byte {first}")
        assert _same_bits(img.numpy(), arr), f"{name}: the image was modified"


def test_pfm_of_the_values_that_straddle_float32_rounding():
    """float32(x) on the device is numpy's astype: ties to even, overflow to inf at FLT_MAX + ulp/2 and not before, fp32
    subnormals kept, underflow to zero at 2^-150 and not above, signed zeros, inf; a NaN stays a NaN."""
    fmax = float(np.finfo(np.float32).max)
    mid = fmax + 2.0 ** 103  # FLT_MAX + ulp/2: a tie between an odd mantissa and 2^128 -> inf
    tiny = 2.0 ** -149
    v = [1 + 2.0 ** -24, np.nextafter(1 + 2.0 ** -24, 0.0), np.nextafter(1 + 2.0 ** -24, 2.0),  # tie -> 1.0 (even), and around it
         1 + 3 * 2.0 ** -24, np.nextafter(1 + 3 * 2.0 ** -24, 0.0), np.nextafter(1 + 3 * 2.0 ** -24, 2.0),  # tie -> up (even)
         fmax, np.nextafter(mid, 0.0), mid, np.nextafter(mid, np.inf), 1e300,
         tiny, 1.5 * tiny, 2.5 * tiny, 2.0 ** -140 * 1.5, 2.0 ** -126 - tiny, 2.0 ** -126, np.nextafter(2.0 ** -126, 0.0),
         tiny / 2, np.nextafter(tiny / 2, 1.0), np.nextafter(tiny / 2, 0.0), 5e-324,  # 2^-150 ties to zero; the next fp64 does not
         0.0, np.inf]
    v = np.array(v + [-x for x in v] + [np.nan, 0.1, 0.2], dtype=np.float64)
    assert v.size % 3 == 0
    arr = v.reshape(1, -1, 3)
    nan_at = np.isnan(v)
    for a in (arr, arr.reshape(-1, 1, 3)):  # one row, and one pixel per row
        for be in (False, True):
            ref = np.frombuffer(R.pfm_payload(a, be), dtype=">f4" if be else "<f4")
            flip = np.isnan(ref)
            for name, make in _legs(a):
                got = np.frombuffer(make().pfm_payload(2 if be else 1), dtype=ref.dtype)
                assert np.array_equal(np.isnan(got), flip), name
                assert got[~flip].tobytes() == ref[~flip].tobytes(), (name, be, got, ref)
    assert nan_at.sum() == 1
    # fp32 input goes through float -> double -> float: every bit pattern above comes back, subnormals included
    with np.errstate(over="ignore"):
        a32 = arr.astype(np.float32)
    keep = ~np.isnan(a32.reshape(-1))
    for name, make in _legs(a32):
        got = np.frombuffer(make().pfm_payload(1), dtype="<f4")
        assert got[keep].tobytes() == a32.reshape(-1)[keep].tobytes() and np.isnan(got[~keep]).all(), name


# ---- luminosity -----------------------------------------------------------------------------------------------------------
def _check_luminosity(arr, delta, label):
    terms = R.luminosity_terms(arr, delta)
    want = 10.0 ** (math.fsum(terms) / terms.size)
    bound = R.luminosity_bound(terms, R.sum_depth(terms.size), L_LOG10, P_HOST)
    seen = {}
    for name, make in _legs(arr):
        seen[name] = make().average_luminosity(delta)
    got = seen["host"]
    rel = abs(got - want) / want
    print(f"luminosity {label}: device {got!r} reference {want!r} rel {rel:.3e} bound {bound:.3e} ({rel / bound:.3f} of it)")
    assert rel <= bound
    assert all(v == got for v in seen.values()), seen  # the sum is deterministic: staged == resident to the bit
    return got, bound


@pytest.mark.parametrize("kind", ["uniform", "hdr"])
@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("size", SIZES, **_ids)
def test_average_luminosity_within_the_derived_bound(size, dtype, kind):
    W, H = size
    _check_luminosity(_image(kind, W, H, dtype), 1e-10, f"{W}x{H} {np.dtype(dtype).name} {kind}")


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
def test_luminosity_with_delta_zero_and_of_a_black_frame(dtype):
    W, H = 2049, 1024  # 257 partials
    _check_luminosity(_image("positive", W, H, dtype), 0.0, "delta 0")
    got, bound = _check_luminosity(np.zeros((H, W, 3), dtype=dtype), 1e-10, "black")
    assert abs(got - 1e-10) / 1e-10 <= bound  # every term is log10(delta): the answer is delta to within pow's error


# ---- tone map -------------------------------------------------------------------------------------------------------------
SCALE = 5.4321  # (explicit: the luminosity sum's rounding does not enter)


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("size", SIZES, **_ids)
def test_tonemap_write_back_is_bit_exact(size, dtype):
    """x * scale and x / (1 + x) are IEEE operations and nothing is contracted: the written-back image equals the reference
    bit for bit; float32 images hold float32(the fp64 result of float64(x))."""
    W, H = size
    arr = _image("hdr", W, H, dtype)
    want_norm, want_clamped = R.tonemap(arr, SCALE, False), R.tonemap(R.tonemap(arr, SCALE, False), 1.0, True)
    want_fused = R.tonemap(arr, SCALE, True)
    for name, make in _legs(arr):
        img = make()
        img.normalize_image(factor=SCALE * 2.0, luminosity=2.0)  # (SCALE * 2 / 2 is SCALE exactly)
        assert _same_bits(img.numpy(), want_norm), f"{name}: normalize"
        img.clamp_image()
        assert _same_bits(img.numpy(), want_clamped), f"{name}: clamp"
        img = make()
        img._tonemap(SCALE, True, 1.0, None, True)  # both in one pass: the fp32 image is rounded once, not twice
        assert _same_bits(img.numpy(), want_fused), f"{name}: normalize + clamp in one call"


def _check_ldr(got, x, gamma, label, cap=True, ref=None):
    want, other, ambiguous = ref if ref is not None else R.ldr_bytes(x, gamma, K_LDR)
    bad = R.ldr_mismatches(got, want, other)
    print(f"LDR {label} gamma {gamma}: {int(ambiguous.sum())} ambiguous of {ambiguous.size}, "
          f"{int((got != want).sum())} on the other accepted side, {int(bad.sum())} wrong")
    if gamma == 1.0:
        assert not ambiguous.any() and np.array_equal(got, want)
    if cap:
        assert ambiguous.mean() <= 1e-6  # a condition on the reference: it must decide all but a millionth by itself
    assert not bad.any(), (np.argwhere(bad)[:5], got[bad][:5], want[bad][:5])


@pytest.mark.parametrize("gamma", [1.0, 2.2])
@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("size", SIZES, **_ids)
def test_ldr_bytes(size, dtype, gamma):
    """(a) uniform values as they are; (b) an HDR frame scaled and clamped in the same call, nothing written back."""
    W, H = size
    a, b = _image("uniform", W, H, dtype), _image("hdr", W, H, dtype)
    ref = R.ldr_bytes(a.astype(np.float64), gamma, K_LDR)
    for name, make in _legs(a):
        img = make()
        _check_ldr(img.ldr_bytes(gamma), None, gamma, f"{W}x{H} {np.dtype(dtype).name} uniform {name}", ref=ref)
        assert _same_bits(img.numpy(), a), f"{name}: ldr_bytes modified the image"
    ref = R.ldr_bytes(R.tonemap_f64(b, SCALE, True), gamma, K_LDR)
    for name, make in _legs(b):
        img = make()
        rgb8 = np.zeros((H, W, 3), dtype=np.uint8)
        img._tonemap(SCALE, True, gamma, rgb8, False)
        _check_ldr(rgb8, None, gamma, f"{W}x{H} {np.dtype(dtype).name} hdr clamped {name}", ref=ref)
        assert _same_bits(img.numpy(), b), f"{name}: write_back = 0 modified the image"


def test_ldr_bytes_on_the_truncation_steps():
    """The inputs that sit on int()'s discontinuities.  gamma 1.0: k/255 and its two fp64 neighbours -- 255 * x is one IEEE
    multiplication, the byte is the reference's, and exactly k/255 gives k.  gamma 2.2: (k/255)**2.2 and neighbours -- each
    value's verdict comes from mpmath; where the exact product is within K ulp of k, k - 1 and k are both right."""
    k = np.arange(256) / 255
    for gamma, centre in ((1.0, k), (2.2, k ** 2.2)):
        x = np.stack([np.nextafter(centre, -1.0), centre, np.nextafter(centre, 2.0)], axis=-1).reshape(1, 256, 3)
        x[0, 0, 0] = 0.0  # (below zero there is nothing to truncate)
        for name, make in _legs(x):
            got = make().ldr_bytes(gamma)
            _check_ldr(got, x, gamma, f"steps {name}", cap=False)
            if gamma == 1.0:
                assert np.array_equal(got[0, :, 1], np.arange(256))
            else:
                assert np.all(np.abs(got[0].astype(int) - np.arange(256)[:, None]) <= 1)


def test_tonemap_beyond_the_byte_range_saturates():
    """clamp = 0 on HDR values: 255 * pow(x, 1/gamma) beyond int's range (1e300, inf), beyond 2^31 at gamma 1.0 only (3e7,
    8.5e6), just beyond a byte (1.0000001): 255.  Negative products and NaN: 0.  With clamp: -0.0 stays -0.0, byte 0."""
    v = np.array([1e300, np.inf, 3e7, 8.5e6, 1.0000001, 1.0, np.nextafter(1.0, 0.0), -1.0, -1e30, -1e-30, np.nan, -0.0,
                  0.0, 0.5, 254.5 / 255, -np.inf, 2.0 ** 31 / 255, 2.0 ** 32 / 255], dtype=np.float64).reshape(1, -1, 3)
    for dtype in DTYPES:
        with np.errstate(over="ignore"):
            a = v.astype(dtype)  # (1e300 is inf as a float32)
        for gamma in (1.0, 2.2):
            want, other, ambiguous = R.ldr_bytes(a.astype(np.float64), gamma, K_LDR)
            assert list(want.reshape(-1)[:5]) == [255] * 5 and list(want.reshape(-1)[7:13]) == [0] * 6
            # (the one value a step below 1.0 is within K ulp of 255 at gamma 2.2 -- in float32 it is 1.0)
            assert int((want != other).sum()) == int(ambiguous.sum()) == (gamma == 2.2 and dtype is np.float64)
            for name, make in _legs(a):
                got = make().ldr_bytes(gamma)
                assert not R.ldr_mismatches(got, want, other).any(), (name, dtype, gamma, got, want)
                assert list(got.reshape(-1)[:5]) == [255] * 5 and list(got.reshape(-1)[7:13]) == [0] * 6
        z = np.array([-0.0, 0.0, 0.25], dtype=dtype).reshape(1, 1, 3)
        for name, make in _legs(z):
            img = make()
            rgb8 = np.full((1, 1, 3), 7, dtype=np.uint8)
            img._tonemap(1.0, True, 2.2, rgb8, True)
            assert _same_bits(img.numpy(), R.tonemap(z, 1.0, True)) and np.signbit(img.numpy()[0, 0, 0]), name
            assert list(rgb8.reshape(-1)[:2]) == [0, 0]


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
def test_the_fused_call_is_the_two_step_result(dtype):
    """scale, clamp, write_back and rgb8 in ONE pt_image_tonemap.  fp64: the image and the bytes of tone mapping first and
    asking for the bytes afterwards, bit for bit.  fp32: the image is float32(x'') as in two steps, but the bytes are those
    of the UNROUNDED fp64 x'' (the kernel converts what it has in registers; csrc/pt_post.h says so) -- the two-step bytes,
    taken from the rounded image, may differ from them by a step, and are compared with their own reference."""
    W, H = 1279, 719
    gamma = 2.2
    arr = _image("hdr", W, H, dtype)
    x64 = R.tonemap_f64(arr, SCALE, True)
    for name, make in _legs(arr):
        fused = make()
        rgb8 = np.zeros((H, W, 3), dtype=np.uint8)
        fused._tonemap(SCALE, True, gamma, rgb8, True)
        assert _same_bits(fused.numpy(), R.tonemap(arr, SCALE, True)), name
        _check_ldr(rgb8, x64, gamma, f"fused {np.dtype(dtype).name} {name}")  # (fp64: x64 is the written-back image itself)
        two = make()
        two._tonemap(SCALE, True, 1.0, None, True)
        assert _same_bits(two.numpy(), fused.numpy()), name
        rgb8_two = two.ldr_bytes(gamma)
        if dtype is np.float64:
            assert np.array_equal(rgb8_two, rgb8), name
        else:
            _check_ldr(rgb8_two, two.numpy().astype(np.float64), gamma, f"two-step float32 {name}")
            print(f"  fused and two-step bytes differ at {int((rgb8_two != rgb8).sum())} of {rgb8.size} values")


# ---- through HdrImage and the render command ----------------------------------------------------------------------------------
def _png_bytes(data: bytes) -> np.ndarray:
    from PIL import Image

    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def test_hdrimage_at_1280x720_against_the_reference():
    from pytracer_amd import hostmodel as hm

    W, H = 1280, 720
    arr = _image("hdr", W, H, np.float64)
    img = hm.HdrImage(W, H)
    img.set_array(arr)
    for endianness, be, sign in ((1, False, "-1.0"), (2, True, "1.0")):
        buf = io.BytesIO()
        img.write_pfm(buf, endianness)
        assert buf.getvalue() == f"PF\n{W} {H}\n{sign}\n".encode() + R.pfm_payload(arr, be)
    terms = R.luminosity_terms(arr)
    lum = R.luminosity(arr)
    assert abs(img.average_luminosity() - lum) / lum <= R.luminosity_bound(terms, R.sum_depth(W * H), L_LOG10, P_HOST)
    img.normalize_image(factor=0.18, luminosity=lum)
    img.clamp_image()
    want = R.tonemap(R.tonemap(arr, 0.18 / lum, False), 1.0, True)
    assert _same_bits(img.array, want)
    for gamma in (1.0, 2.2):
        png = io.BytesIO()
        img.write_ldr_image(png, "PNG", gamma)
        _check_ldr(_png_bytes(png.getvalue()), want, gamma, "HdrImage")


def test_render_command_at_1280x720_against_the_reference(tmp_path):
    """The files `render` writes from its HBM-resident frame against post_reference applied to the same frame rendered to
    the host (the render kernels are other tests' business; none of the post-processing kernels touches this copy).
    The command's scale is 1 / (the device's own luminosity): that value is known to the derived bound, the bytes are
    monotone in it, so every byte must lie between the reference's bytes at the two ends of the bound -- at gamma 1.0
    nothing else is uncertain."""
    from click.testing import CliRunner

    from pytracer_amd import cli as ptcli
    from pytracer_amd import hostmodel as hm
    from pytracer_amd.tracer import GpuImageTracer

    W, H = 1280, 720
    pfm, png = str(tmp_path / "o.pfm"), str(tmp_path / "o.png")
    r = CliRunner().invoke(ptcli.cli, ["render", "--width", str(W), "--height", str(H), "--algorithm", "flat", "--pfm-output", pfm,
                                       "--png-output", png, "-d", "clock:150", "builtin:demo"])
    assert r.exit_code == 0, r.output
    job = ptcli.plan_render(W, H, "flat", 10, 3, 45, 54, 1, ["clock:150"], "builtin:demo")
    image = hm.HdrImage(W, H)
    tracer = GpuImageTracer(image=image, camera=job.camera, samples_per_side=job.samples_per_side, device=0, pcg_mode="auto")
    tracer.fire_all_rays(job.renderer)
    tracer.close()
    frame = np.array(image.array)
    assert frame.min() >= 0.0 and len(np.unique(frame.reshape(-1, 3), axis=0)) > 3  # (a picture, not a constant)
    with open(pfm, "rb") as f:
        assert f.read() == f"PF\n{W} {H}\n-1.0\n".encode() + R.pfm_payload(frame, False)
    terms = R.luminosity_terms(frame)
    lum = R.luminosity(frame)
    bound = R.luminosity_bound(terms, R.sum_depth(W * H), L_LOG10, P_HOST)
    ends = []
    for lum_end in (lum * (1 + bound), lum * (1 - bound)):  # (the larger luminosity gives the smaller bytes)
        toned = R.tonemap(R.tonemap(frame, 1.0 / lum_end, False), 1.0, True)
        ends.append(R.ldr_bytes(toned, 1.0, K_LDR)[0])
    with open(png, "rb") as f:
        got = _png_bytes(f.read())
    print(f"render: {int((ends[0] != ends[1]).sum())} of {got.size} bytes depend on the luminosity's last bits")
    assert np.all(ends[0] <= ends[1]) and (ends[0] != ends[1]).mean() <= 1e-6
    assert np.all((ends[0] <= got) & (got <= ends[1]))


# ---- errors ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_leave_the_image_alone():
    L = _lib.lib()
    arr = _image("uniform", 3, 1, np.float64).copy()
    before = arr.copy()
    p = arr.ctypes.data_as(C.c_void_p)
    out = np.full(64, 0x5A, dtype=np.uint8)
    po = out.ctypes.data_as(C.c_void_p)
    lum = C.c_double(-1.0)
    F64 = abi.OUT_F64
    bad = [(p, F64, 0, 1), (p, F64, 3, 0), (p, F64, -3, 1), (p, 77, 3, 1), (None, F64, 3, 1)]
    for img, fmt, w, h in bad:
        assert L.pt_image_pack_pfm(0, img, fmt, w, h, 0, po, None) == PT_ERR_INVALID
        assert L.pt_image_average_luminosity(0, img, fmt, w, h, 1e-10, C.byref(lum), None) == PT_ERR_INVALID
        assert L.pt_image_tonemap(0, img, fmt, w, h, 2.0, 1, 1.0, po, 1, None) == PT_ERR_INVALID
    for gamma in (0.0, -2.2, float("nan")):
        assert L.pt_image_tonemap(0, p, F64, 3, 1, 2.0, 1, gamma, po, 1, None) == PT_ERR_INVALID
    assert L.pt_image_pack_pfm(0, p, F64, 3, 1, 0, None, None) == PT_ERR_INVALID
    assert L.pt_image_average_luminosity(0, p, F64, 3, 1, 1e-10, None, None) == PT_ERR_INVALID
    assert _same_bits(arr, before) and np.all(out == 0x5A) and lum.value == -1.0
    # ... and gamma is not looked at when no bytes are asked for
    assert L.pt_image_tonemap(0, p, F64, 3, 1, 2.0, 0, 0.0, None, 1, None) == 0
    assert _same_bits(arr, before * 2.0)
