"""SURVEY.md §8f next-3 — HdrImage post-processing (write_pfm, average_luminosity, normalize, clamp, LDR).

CPU: the oracle against the reference's golden outputs (bit-exact) and its known-answer vectors.
GPU: the device kernels (through the C-ABI) against the same goldens."""
from io import BytesIO

import numpy as np
import pytest

from tests import post_reference as R
from tests import util

# test_all.py:112-143: the reference's own PFM vectors for the 3x2 image below
LE_REFERENCE_BYTES = bytes([
    0x50, 0x46, 0x0A, 0x33, 0x20, 0x32, 0x0A, 0x2D, 0x31, 0x2E, 0x30, 0x0A, 0x00, 0x00, 0xC8, 0x42,
    0x00, 0x00, 0x48, 0x43, 0x00, 0x00, 0x96, 0x43, 0x00, 0x00, 0xC8, 0x43, 0x00, 0x00, 0xFA, 0x43,
    0x00, 0x00, 0x16, 0x44, 0x00, 0x00, 0x2F, 0x44, 0x00, 0x00, 0x48, 0x44, 0x00, 0x00, 0x61, 0x44,
    0x00, 0x00, 0x20, 0x41, 0x00, 0x00, 0xA0, 0x41, 0x00, 0x00, 0xF0, 0x41, 0x00, 0x00, 0x20, 0x42,
    0x00, 0x00, 0x48, 0x42, 0x00, 0x00, 0x70, 0x42, 0x00, 0x00, 0x8C, 0x42, 0x00, 0x00, 0xA0, 0x42,
    0x00, 0x00, 0xB4, 0x42])
BE_REFERENCE_BYTES = bytes([
    0x50, 0x46, 0x0A, 0x33, 0x20, 0x32, 0x0A, 0x31, 0x2E, 0x30, 0x0A, 0x42, 0xC8, 0x00, 0x00, 0x43,
    0x48, 0x00, 0x00, 0x43, 0x96, 0x00, 0x00, 0x43, 0xC8, 0x00, 0x00, 0x43, 0xFA, 0x00, 0x00, 0x44,
    0x16, 0x00, 0x00, 0x44, 0x2F, 0x00, 0x00, 0x44, 0x48, 0x00, 0x00, 0x44, 0x61, 0x00, 0x00, 0x41,
    0x20, 0x00, 0x00, 0x41, 0xA0, 0x00, 0x00, 0x41, 0xF0, 0x00, 0x00, 0x42, 0x20, 0x00, 0x00, 0x42,
    0x48, 0x00, 0x00, 0x42, 0x70, 0x00, 0x00, 0x42, 0x8C, 0x00, 0x00, 0x42, 0xA0, 0x00, 0x00, 0x42,
    0xB4, 0x00, 0x00])
# test_all.py:177-186: the image those bytes encode
REF_IMAGE = np.array([[[1.0e1, 2.0e1, 3.0e1], [4.0e1, 5.0e1, 6.0e1], [7.0e1, 8.0e1, 9.0e1]],
                      [[1.0e2, 2.0e2, 3.0e2], [4.0e2, 5.0e2, 6.0e2], [7.0e2, 8.0e2, 9.0e2]]])
LE_HEADER, BE_HEADER = b"PF\n3 2\n-1.0\n", b"PF\n3 2\n1.0\n"


def test_oracle_pfm_known_answer(oracle):
    assert LE_HEADER + oracle.pack_pfm(REF_IMAGE, False) == LE_REFERENCE_BYTES
    assert BE_HEADER + oracle.pack_pfm(REF_IMAGE, True) == BE_REFERENCE_BYTES


def test_oracle_luminosity_known_answers(oracle):
    img = np.array([[[0.5e1, 1.0e1, 1.5e1], [0.5e3, 1.0e3, 1.5e3]]])  # test_all.py:239-246
    assert oracle.average_luminosity(img, delta=0.0) == pytest.approx(100.0)
    toned, _ = oracle.tonemap(img, 1000.0 / 100.0, clamp=False)  # test_all.py:248-256
    assert np.allclose(toned, [[[0.5e2, 1.0e2, 1.5e2], [0.5e4, 1.0e4, 1.5e4]]])
    clamped, _ = oracle.tonemap(img, 1.0, clamp=True)
    assert np.all((clamped >= 0) & (clamped <= 1))


@pytest.mark.parametrize("tag", ["a", "b"])
def test_oracle_postprocess_golden(oracle, tag):
    g = util.load("g10_postprocess")
    px = g[f"{tag}_pixels"]
    h, w = px.shape[:2]
    hdr = f"PF\n{w} {h}\n".encode()
    assert hdr + b"-1.0\n" + oracle.pack_pfm(px, False) == g[f"{tag}_pfm_le"].tobytes()
    assert hdr + b"1.0\n" + oracle.pack_pfm(px, True) == g[f"{tag}_pfm_be"].tobytes()
    lum = oracle.average_luminosity(px)
    assert lum == float(g[f"{tag}_lum"])
    assert oracle.average_luminosity(px, 1e-3) == float(g[f"{tag}_lum_delta0"])
    toned, ldr = oracle.tonemap(px, 1.0 / lum, clamp=True, gamma=1.0)
    assert util.bits_equal(toned, g[f"{tag}_toned"])
    assert np.array_equal(ldr, g[f"{tag}_ldr_g10"])
    _, ldr22 = oracle.tonemap(g[f"{tag}_toned"], 1.0, clamp=False, gamma=2.2)
    assert np.array_equal(ldr22, g[f"{tag}_ldr_g22"])


# ---- tests/post_reference.py, the judge of tests/test_gpu_postprocess.py, pinned to the oracle and to the goldens ------------
K_LIBM = 2.0  # glibc's pow is within 1 ulp: a product within 2 ulp of an integer is left to mpmath (post_reference.ldr_bytes)


def _random_frames():
    rng = np.random.default_rng(7)
    hdr = 10.0 ** rng.uniform(-6.0, 4.0, (61, 173, 3))
    hdr[rng.random((61, 173)) < 0.25] = 0.0
    return {"uniform": rng.random((61, 173, 3)), "hdr": hdr}


def _pinned_frames():
    g = util.load("g10_postprocess")
    return {"a": g["a_pixels"], "b": g["b_pixels"], **_random_frames()}


@pytest.mark.parametrize("tag", ["a", "b"])
def test_reference_reproduces_the_goldens(tag):
    g = util.load("g10_postprocess")
    px = g[f"{tag}_pixels"]
    h, w = px.shape[:2]
    hdr = f"PF\n{w} {h}\n".encode()
    assert hdr + b"-1.0\n" + R.pfm_payload(px, False) == g[f"{tag}_pfm_le"].tobytes()
    assert hdr + b"1.0\n" + R.pfm_payload(px, True) == g[f"{tag}_pfm_be"].tobytes()
    toned = R.tonemap(R.tonemap(px, 1.0 / float(g[f"{tag}_lum"]), False), 1.0, True)
    assert util.bits_equal(toned, g[f"{tag}_toned"]) and util.bits_equal(R.tonemap(px, 1.0 / float(g[f"{tag}_lum"]), True), toned)
    want, other, ambiguous = R.ldr_bytes(toned, 1.0, K_LIBM)
    assert not ambiguous.any() and np.array_equal(want, g[f"{tag}_ldr_g10"])
    want, other, ambiguous = R.ldr_bytes(toned, 2.2, K_LIBM)
    assert ambiguous.mean() <= 1e-6 and not R.ldr_mismatches(g[f"{tag}_ldr_g22"], want, other).any()
    assert np.array_equal(want[~ambiguous], g[f"{tag}_ldr_g22"][~ambiguous])


@pytest.mark.parametrize("name", ["a", "b", "uniform", "hdr"])
def test_reference_reproduces_the_oracle(oracle, name):
    px = _pinned_frames()[name]
    for be in (False, True):
        assert R.pfm_payload(px, be) == oracle.pack_pfm(px, be)
    for scale, clamp in ((5.4321, False), (5.4321, True), (1.0, True)):
        for gamma in (1.0, 2.2):
            toned, ldr = oracle.tonemap(px, scale, clamp=clamp, gamma=gamma)
            assert util.bits_equal(toned, R.tonemap(px, scale, clamp))
            want, other, ambiguous = R.ldr_bytes(R.tonemap_f64(px, scale, clamp), gamma, K_LIBM)
            assert ambiguous.mean() <= 1e-6 and not R.ldr_mismatches(ldr, want, other).any()
            assert np.array_equal(want[~ambiguous], ldr[~ambiguous]) and (gamma != 1.0 or not ambiguous.any())
    # float32 frames: float32(the fp64 result of float64(x)), which is what the oracle computes on the widened frame
    px32 = px.astype(np.float32)
    toned, _ = oracle.tonemap(px32.astype(np.float64), 5.4321, clamp=True)
    assert np.array_equal(R.tonemap(px32, 5.4321, True).view(np.uint32), toned.astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("name", ["a", "b", "uniform", "hdr"])
@pytest.mark.parametrize("delta", [1e-10, 1e-3])
def test_reference_luminosity_against_the_oracles_sequential_sum(oracle, name, delta):
    """The bound of post_reference.luminosity_bound for the oracle: one chain of n additions (depth n); glibc's log10 is
    within 2 ulp (its manual's figure for x86-64) = 4 U|t| of the exact value and the reference's terms within 1 U|t|:
    L = 5; both end in the same pow, within 1 ulp."""
    px = _pinned_frames()[name]
    terms = R.luminosity_terms(px, delta)
    want, got = R.luminosity(px, delta), oracle.average_luminosity(px, delta)
    bound = R.luminosity_bound(terms, terms.size, 5.0, 1.0)
    print(f"{name}: oracle {got!r} reference {want!r} rel {abs(got - want) / want:.3e} bound {bound:.3e}")
    assert abs(got - want) / want <= bound


def test_reference_luminosity_known_answers():
    img = np.array([[[0.5e1, 1.0e1, 1.5e1], [0.5e3, 1.0e3, 1.5e3]]])  # test_all.py:239-246
    assert R.luminosity(img, delta=0.0) == pytest.approx(100.0, rel=1e-15)
    assert R.sum_depth(1) == 1 + 8 + 1 + 8 and R.sum_depth(3840 * 2160) == 32 + 8 + 4 + 8 and R.sum_depth(8193) == 32 + 8 + 1 + 8


def test_reference_terms_and_host_pow_against_mpmath():
    """The fp64 terms are within 1 U|t| of the exact log10 (extended precision, rounded once), Python's 10 ** y -- libm's
    pow, which pt_image_average_luminosity ends in too -- within 1 ulp of the exact power: both at 50 digits."""
    pytest.importorskip("mpmath")
    for name, px in _random_frames().items():
        px = px[:20]
        lum = 1e-10 + (px.reshape(-1, 3).max(axis=1) + px.reshape(-1, 3).min(axis=1)) / 2
        ulp, units = R.exact_distance("log10", R.luminosity_terms(px), lum)
        print(f"{name}: terms within {ulp:.3f} ulp, {units:.3f} U|t|")
        assert units <= 1.0
    y = np.random.default_rng(5).uniform(-10.0, 4.0, 5000)
    ulp, _ = R.exact_distance("pow", np.array([10.0 ** v for v in y]), np.full_like(y, 10.0), y)
    print(f"10 ** y on -10..4: {ulp:.3f} ulp")
    assert ulp <= 1.0
    # ... and the extended-precision stand-in that measures the device's functions agrees with the 50 digits
    x = 10.0 ** np.random.default_rng(6).uniform(-10.0, 4.0, 2000)
    got = np.log10(x)
    a, b = R.distance(got, np.log10(x.astype(np.longdouble))), R.exact_distance("log10", got, x)
    assert abs(a[0] - b[0]) <= 2.0 ** -9 and abs(a[1] - b[1]) <= 2.0 ** -8


def test_reference_ldr_bytes_at_the_steps_and_away_from_them(oracle):
    k = np.arange(256)
    want, other, ambiguous = R.ldr_bytes(k / 255, 1.0, 64.0)
    assert np.array_equal(want, k) and np.array_equal(other, k) and not ambiguous.any()
    assert [int(255 * (i / 255)) for i in range(256)] == list(range(256))
    # random values: the reference decides all but a millionth by itself, even at 64 ulp
    x = np.random.default_rng(9).random(2_000_000)
    want, other, ambiguous = R.ldr_bytes(x, 2.2, 64.0)
    assert ambiguous.mean() <= 1e-6
    _, ldr = oracle.tonemap(x.reshape(-1, 1, 1), 1.0, clamp=False, gamma=2.2)
    assert not R.ldr_mismatches(ldr.reshape(-1), want, other).any()
    # on the steps of gamma 2.2 fp64 cannot decide: every verdict is mpmath's, and the oracle's byte is an accepted one
    centre = (k / 255) ** 2.2
    for x in (np.nextafter(centre, 0.0), centre, np.nextafter(centre, 2.0)):
        want, other, ambiguous = R.ldr_bytes(x, 2.2, K_LIBM)
        assert ambiguous[1:255].all() and np.all((want == k) | (want == np.maximum(k - 1, 0)))
        assert np.all((other == k) | (other == np.maximum(k - 1, 0)))
        _, ldr = oracle.tonemap(x.reshape(-1, 1, 1), 1.0, clamp=False, gamma=2.2)
        assert not R.ldr_mismatches(ldr.reshape(-1), want, other).any()


@pytest.mark.parametrize("gamma", [1.0, 2.2])
def test_oracle_saturates_beyond_the_byte_range(oracle, gamma):
    """255 * pow(x, 1/gamma) beyond int's range used to go through (int)v, undefined in C (the oracle returned 0 for 1e300,
    inf, and 3e7 at gamma 1.0): the product saturates as a double.  In range nothing changed (the goldens above)."""
    x = np.array([1e300, np.inf, 3e7, 8.5e6, 1.0000001, 2.0 ** 31 / 255, 2.0 ** 32 / 255, 1.0, np.nan, -1.0, -1e300, -0.0,
                  0.0, 254.999 / 255 if gamma == 1.0 else 0.999]).reshape(-1, 1, 1)
    _, ldr = oracle.tonemap(x, 1.0, clamp=False, gamma=gamma)
    assert list(ldr.reshape(-1)) == [255] * 8 + [0] * 5 + [254]
    want, other, _ = R.ldr_bytes(x, gamma, K_LIBM)
    assert np.array_equal(want, ldr) and np.array_equal(other, ldr)


# ---- device ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_pfm_known_answer():
    from pytracer_amd.postprocess import BIG_ENDIAN, LITTLE_ENDIAN, DeviceImage

    for dtype in (np.float64, np.float32):
        img = DeviceImage.from_numpy(REF_IMAGE.astype(dtype))
        buf = BytesIO()
        img.write_pfm(buf, LITTLE_ENDIAN)
        assert buf.getvalue() == LE_REFERENCE_BYTES
        buf = BytesIO()
        img.write_pfm(buf, BIG_ENDIAN)
        assert buf.getvalue() == BE_REFERENCE_BYTES


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["a", "b"])
def test_device_postprocess_golden(tag):
    from pytracer_amd.postprocess import BIG_ENDIAN, DeviceImage

    g = util.load("g10_postprocess")
    px = g[f"{tag}_pixels"]
    img = DeviceImage.from_numpy(px)
    buf = BytesIO()
    img.write_pfm(buf)
    assert buf.getvalue() == g[f"{tag}_pfm_le"].tobytes()  # byte-exact
    buf = BytesIO()
    img.write_pfm(buf, BIG_ENDIAN)
    assert buf.getvalue() == g[f"{tag}_pfm_be"].tobytes()
    # the reference sums log10 sequentially; the device sums pairwise: equal to rounding of the sum
    lum = img.average_luminosity()
    assert lum == pytest.approx(float(g[f"{tag}_lum"]), rel=1e-12)
    img.normalize_image(factor=1.0)
    img.clamp_image()
    assert util.rel_err(img.numpy(), g[f"{tag}_toned"]).max() <= 1e-12
    for gamma, key in ((1.0, "g10"), (2.2, "g22")):
        ldr = img.ldr_bytes(gamma).astype(np.int32)
        diff = np.abs(ldr - g[f"{tag}_ldr_{key}"])
        # int() truncation is discontinuous: allow a unit step on a handful of values (pow is not bit-equal)
        assert diff.max() <= 1 and (diff > 0).mean() < 1e-3
    # with the golden's own luminosity handed in, nothing is left to round differently: multiply and divide are IEEE
    # operations, and at gamma 1.0 pow(x, 1.0) is x
    img = DeviceImage.from_numpy(px)
    img.normalize_image(factor=1.0, luminosity=float(g[f"{tag}_lum"]))
    img.clamp_image()
    assert util.bits_equal(img.numpy(), g[f"{tag}_toned"])
    assert np.array_equal(img.ldr_bytes(1.0), g[f"{tag}_ldr_g10"])
    want, other, ambiguous = R.ldr_bytes(g[f"{tag}_toned"], 2.2, 5.0)  # (K as in tests/test_gpu_postprocess.py)
    assert ambiguous.mean() <= 1e-6 and not R.ldr_mismatches(img.ldr_bytes(2.2), want, other).any()


@pytest.mark.gpu
def test_device_resident_tensor_path():
    """A frame left in HBM by pt_render_device (a torch tensor) goes through the same kernels in place."""
    import torch

    from pytracer_amd.postprocess import DeviceImage

    g = util.load("g10_postprocess")
    t = torch.from_numpy(g["a_pixels"]).cuda().contiguous()
    img = DeviceImage(t)
    buf = BytesIO()
    img.write_pfm(buf)
    assert buf.getvalue() == g["a_pfm_le"].tobytes()
    img.normalize_image(factor=1.0)
    img.clamp_image()
    assert util.rel_err(t.cpu().numpy(), g["a_toned"]).max() <= 1e-12  # modified in HBM, in place
    t2 = torch.from_numpy(g["a_pixels"]).cuda().contiguous()
    img = DeviceImage(t2)
    img.normalize_image(factor=1.0, luminosity=float(g["a_lum"]))
    img.clamp_image()
    assert util.bits_equal(t2.cpu().numpy(), g["a_toned"])  # ... to the bit when the scale is given
    assert np.array_equal(img.ldr_bytes(1.0), g["a_ldr_g10"])


@pytest.mark.gpu
def test_hdrimage_standin_methods():
    from pytracer_amd import hostmodel as hm

    g = util.load("g10_postprocess")
    px = g["a_pixels"]
    img = hm.HdrImage(px.shape[1], px.shape[0])
    img.set_array(px)
    buf = BytesIO()
    img.write_pfm(buf)
    assert buf.getvalue() == g["a_pfm_le"].tobytes()
    assert img.average_luminosity() == pytest.approx(float(g["a_lum"]), rel=1e-12)
    img.normalize_image(factor=1.0)
    img.clamp_image()
    assert util.rel_err(img.array, g["a_toned"]).max() <= 1e-12
    png = BytesIO()
    img.write_ldr_image(png, "PNG")
    assert png.getvalue()[:8] == b"\x89PNG\r\n\x1a\n"
