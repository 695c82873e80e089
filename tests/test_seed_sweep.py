"""The seed sweep (tests/seed_sweep.py) on the CPU: the conditions that make tests/test_gpu_seeds.py mean something.

* The generators of this project (``hostmodel.PCG``, ``oracle.Pcg``) against the reference's own over the whole 64-bit range
  of both seeds and for ints outside it (tests/golden/g15_pcg_wide.npz), and the host plumbing with such ints.
* The oracle's frames across the crossing against a derivation that shares nothing with ``pto_render``'s seeding: the
  sequence number summed in Python, ``hostmodel.PCG`` for the jitter, one ``radiance`` call for the pixel.
* Sensitivity: a frame under a swept pair differs, on both sides of the crossing, from the frames a truncated or shifted
  seed would give.  Without this a device frame equal to the oracle's would say nothing about the top 32 bits.
* tests/test_variant_catalog.py's real-work assertions for the swept params of every path-tracer case.
"""
import os

import numpy as np
import pytest

from pytracer_amd import abi, flatten
from pytracer_amd import hostmodel as hm
from tests import seed_sweep as ss
from tests import util
from tests import variant_catalog as vc
from tests.test_cli import reference_importable  # noqa: F401  (fixture: the reference's parser on sys.path, where present)
from tests.test_golden_regen import REFERENCE
from tests.test_golden_regen import test_regenerated_fixture_equals_the_committed_one as _regenerated_equals_committed
from tests.test_variant_catalog import test_case_does_real_work_on_the_oracle as _real_work

M64 = ss.M64
OUT_OF_RANGE = [-1, -(2**63), 2**64 + 5, 2**70 + 3]


# ---- the generators against the reference's, over the whole range ----------------------------------------------------------
@pytest.fixture(scope="module")
def g15():
    d = util.load("g15_pcg_wide")
    rows = []
    for i in range(len(d["seeds"])):
        rows.append(dict(raw=(int(d["raw"][i][0]), int(d["raw"][i][1])), seeds=(int(d["seeds"][i][0]), int(d["seeds"][i][1])),
                         valid=bool(d["valid"][i]), state=int(d["state"][i]), inc=int(d["inc"][i]),
                         outputs=[int(v) for v in d["outputs"][i]]))
    return rows


def test_fixture_holds_the_cases(g15):
    states = [ss.PAIRS[n][0] for n in ss.SEED_NAMES]
    seqs = [54, 2**32 - 1, 2**32, 2**63 - 1, 2**63, 2**64 - 1]
    want = [(s, q) for s in states for q in seqs] + [(x, 54) for x in OUT_OF_RANGE] + [(45, x) for x in OUT_OF_RANGE]
    assert [r["raw"] for r in g15] == want
    assert all(r["seeds"] == (r["raw"][0] & M64, r["raw"][1] & M64) for r in g15)
    # the one row the reference has no answer for: its constructor raises (a negative shift count in the output it discards)
    assert [r["raw"] for r in g15 if not r["valid"]] == [(-(2**63), 54)]


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference is not present here")
def test_fixture_regenerates_from_the_reference(tmp_path):
    _regenerated_equals_committed(tmp_path, "g15", ["g15_pcg_wide"])


def _draw(g, n=8):
    return [g.random() for _ in range(n)]


def test_both_generators_reproduce_the_reference_on_reduced_seeds(g15, oracle):
    for r in (r for r in g15 if r["valid"]):
        for cls in (hm.PCG, oracle.Pcg):
            g = cls(*r["seeds"])
            assert (g.state, g.inc) == (r["state"], r["inc"]), (cls.__name__, r["raw"])
            assert _draw(g) == r["outputs"], (cls.__name__, r["raw"])


def test_host_generator_reproduces_the_reference_on_raw_ints(g15):
    for r in g15:
        g = hm.PCG(*r["raw"])
        if r["valid"]:
            assert (g.state, g.inc, _draw(g)) == (r["state"], r["inc"], r["outputs"]), r["raw"]
        else:  # where the reference raises, this one is the modular generator
            h = hm.PCG(*r["seeds"])
            assert (g.state, g.inc, _draw(g)) == (h.state, h.inc, _draw(h))


class _StateOnly:
    """What the reference's PCG is to the flattener: (state, inc) and nothing remembered."""

    def __init__(self, state, inc):
        self.state, self.inc = state, inc


def test_recover_seeds_round_trips(g15):
    for r in (r for r in g15 if r["valid"]):
        s, q = flatten.recover_seeds(_StateOnly(r["state"], r["inc"]))
        # bit 63 of a sequence number is not in (state, inc): the generator's definition drops it
        assert (s, q) == (r["seeds"][0], r["seeds"][1] & (2**63 - 1)), r["raw"]
        g = hm.PCG(s, q)
        assert (g.state, g.inc, _draw(g)) == (r["state"], r["inc"], r["outputs"]), r["raw"]
        # ... and further down the stream: the seeds of the generator that starts where this one has got to
        h = hm.PCG(*r["seeds"])
        _draw(h, 5)
        g = hm.PCG(*flatten.recover_seeds(_StateOnly(h.state, h.inc)))
        assert (g.state, g.inc) == (h.state, h.inc) and _draw(g) == _draw(h)
        # a generator that remembers its seeds gives them as they were; the boundary reduces them
        raw = flatten.recover_seeds(hm.PCG(*r["raw"]), constructed=True)
        assert raw == r["raw"]
        p = abi.make_params(4, 4, abi.RENDERER_PATHTRACER, path_state=raw[0], path_seq=raw[1])
        assert (p.path_state, p.path_seq) == r["seeds"]


# ---- host plumbing with ints outside [0, 2^64): reduced mod 2^64 ---------------------------------------------------------
WIDE_INTS = OUT_OF_RANGE + [2**64 - 1, 2**63, 2**32]


@pytest.mark.parametrize("x", WIDE_INTS)
def test_make_params_reduces_every_seed_mod_2_64(x):
    p = abi.make_params(8, 8, abi.RENDERER_FLAT, jitter_state=x, jitter_seq=x + 1, path_state=x + 2, path_seq=x + 3)
    assert (p.jitter_state, p.jitter_seq, p.path_state, p.path_seq) == tuple((x + k) & M64 for k in range(4))
    q = abi.copy_params(p, path_seq=x)
    assert q.path_seq == x & M64 and q.path_state == p.path_state


@pytest.mark.parametrize("mode", [abi.PCG_SEQ, abi.PCG_PIXEL, abi.PCG_SAMPLE])
@pytest.mark.parametrize("x", WIDE_INTS)
def test_renderer_params_reduce_mod_2_64(x, mode):
    world = hm.World()
    pt = hm.PathTracer(world, pcg=hm.PCG(x, x + 1))
    par = flatten.renderer_params(pt, 8, 6, samples_per_side=2, tracer_pcg=hm.PCG(x + 2, x + 3), pcg_mode=mode)
    want = tuple((x + k) & M64 for k in range(4))
    if mode == abi.PCG_SEQ:  # (solved for from (state, inc), which hold no bit 63 of a sequence number)
        want = (want[0], want[1] & (2**63 - 1), want[2], want[3] & (2**63 - 1))
    assert (par.path_state, par.path_seq, par.jitter_state, par.jitter_seq) == want
    # a generator that has been drawn from: the SEQ frame goes on where it stands
    t = hm.PCG(x, x + 1)
    _draw(t, 7)
    par = flatten.renderer_params(hm.FlatRenderer(world), 8, 6, samples_per_side=2, tracer_pcg=t, pcg_mode=abi.PCG_SEQ)
    g = hm.PCG(par.jitter_state, par.jitter_seq)
    assert (g.state, g.inc) == (t.state, t.inc)


def _plan_params(init_state, init_seq, scene, mode):
    from pytracer_amd.cli import plan_render

    job = plan_render(16, 12, "pathtracing", 3, 2, init_state, init_seq, 4, (), scene)
    return flatten.renderer_params(job.renderer, 16, 12, samples_per_side=job.samples_per_side, pcg_mode=mode)


@pytest.mark.parametrize("x", WIDE_INTS)
def test_render_command_reduces_its_seeds_mod_2_64(x):
    for mode in (abi.PCG_PIXEL, abi.PCG_SAMPLE):
        got = _plan_params(x, x + 1, "builtin:c3", mode)
        want = _plan_params(x & M64, (x + 1) & M64, "builtin:c3", mode)
        assert bytes(got) == bytes(want) and (got.path_state, got.path_seq) == (x & M64, (x + 1) & M64)


@pytest.mark.parametrize("x", WIDE_INTS)
def test_render_command_reduces_its_seeds_for_the_reference_classes(reference_importable, x):  # noqa: F811
    """A scene file is rendered with pytracer's own PCG, which raises from its first draw for ``PCG(-(2**63), 54)``: the
    command reduces before it builds one.  Its (state, inc) hold no bit 63 of the sequence number (the generator drops it)."""
    from tests.test_cli import REF_DEMO

    got = _plan_params(x, x + 1, REF_DEMO, abi.PCG_SAMPLE)
    assert (got.path_state, got.path_seq) == (x & M64, (x + 1) & (2**63 - 1))


@pytest.mark.parametrize("x", WIDE_INTS)
def test_tracer_hit_params_and_its_stream_behind_a_frame(x):
    """``GpuImageTracer``'s hit-frame params (pytracer_amd/tracer.py) and where its generator stands behind a SEQ frame.
    pytracer_amd/pixels.py holds no seed."""
    from pytracer_amd.tracer import GpuImageTracer

    W, H, S = 3, 2, 2
    for mode in ("pixel", "sample"):
        t = GpuImageTracer(hm.HdrImage(W, H), hm.PerspectiveCamera(aspect_ratio=1.5), samples_per_side=S, pcg=hm.PCG(x, x + 1), pcg_mode=mode)
        p = t._hits_params()
        assert (p.path_state, p.path_seq, p.jitter_state, p.jitter_seq) == (x & M64, (x + 1) & M64) * 2
    t = GpuImageTracer(hm.HdrImage(W, H), hm.PerspectiveCamera(aspect_ratio=1.5), samples_per_side=S, pcg=hm.PCG(x, x + 1), pcg_mode="seq")
    p = t._hits_params()
    g = hm.PCG(p.jitter_state, p.jitter_seq)
    assert (g.state, g.inc) == (t.pcg.state, t.pcg.inc) and p.jitter_state == x & M64
    t._advance_behind_hits()
    _draw(g, 2 * W * H * S * S)
    assert t.pcg.state == g.state


# ---- the oracle's frames, cached for everything below ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def frames(oracle):
    """``frames(case, mode, state, seq)`` -> the oracle's frame (x*x mode) and ray count of ``case`` under (state, seq); ``mode``
    None: the case's own alignment.  Each frame is rendered once for this file (the sensitivity condition asks for four per
    swept frame: some 350 small frames in all) and let go when the file has run."""
    cache = {}

    def image(case, mode, state, seq):
        key = (case.id, mode, state, seq)
        if key not in cache:
            base = vc.params(case)
            if mode == abi.PCG_SEQ:
                base = abi.copy_params(base, pcg_mode=abi.PCG_SEQ)
            try:
                cache[key] = oracle.render(vc.scene(case), vc.camera(case), ss.with_seeds(base, state, seq), sqr_mode=oracle.SQR_MUL)
            finally:
                oracle.set_sqr_mode(oracle.SQR_POW)
        return cache[key]

    yield image
    cache.clear()


def test_swept_params_change_the_seeds_only():
    for cid, name, mode in ss.SWEEP:
        case = vc.BY_ID[cid]
        base, p = vc.params(case), ss.params(case, name, mode)
        state, seq = ss.seeds(case, name, mode)
        assert 0 <= state < 2**64 and 0 <= seq < 2**64
        if mode == abi.PCG_SEQ:
            assert (p.pcg_mode, p.jitter_state, p.jitter_seq, p.path_state, p.path_seq) == (abi.PCG_SEQ, state, seq) + ss.UNUSED
            assert p.renderer != abi.RENDERER_PATHTRACER and p.samples_per_side > 0 and p.n_ranks == 1
        else:
            assert (p.pcg_mode, p.path_state, p.path_seq, p.jitter_state, p.jitter_seq) == (base.pcg_mode, state, seq) + ss.UNUSED
            # the frame draws numbers, and the sum reaches the boundary exactly at the crossing pixel, inside the rows rendered
            assert p.samples_per_side > 0 or p.renderer == abi.RENDERER_PATHTRACER
            row, col = ss.crossing_pixel(case)
            rows = vc.rows(case)
            assert rows[0] < row < rows[-1] and 0 < col < p.width - 1
            boundary = ss.PAIRS[name][1]
            if boundary is not None:
                assert seq + ss.crossing_index(p, row, col) == boundary
                last = ss.nsamp(p) - 1 if p.pcg_mode == abi.PCG_SAMPLE else 0  # (the last generator of the pixel before it)
                assert seq + ss.crossing_index(p, row, col - 1) + last == boundary - 1
        same = abi.copy_params(p, pcg_mode=base.pcg_mode, jitter_state=base.jitter_state, jitter_seq=base.jitter_seq,
                               path_state=base.path_state, path_seq=base.path_seq)
        assert bytes(same) == bytes(base)
    # every case of the issue's list, both alignments on every kernel family that has both
    modes = {fam: {vc.params(vc.BY_ID[c]).pcg_mode for c in ids} for fam, ids in (("simple", ss.SIMPLE), ("tile", ss.TILE), ("path", ss.PATH))}
    assert all(m == {abi.PCG_PIXEL, abi.PCG_SAMPLE} for m in modes.values())
    assert any(vc.params(vc.BY_ID[c]).pcg_mode == abi.PCG_SAMPLE and vc.params(vc.BY_ID[c]).samples_per_side > 1 for c in ss.TILE)
    assert set(ss.SEQ_CASE_IDS) & set(ss.SIMPLE) and set(ss.SEQ_CASE_IDS) & set(ss.TILE)


# ---- the oracle across the crossing, against an independent derivation -----------------------------------------------------
@pytest.mark.parametrize("name", ss.CROSSING_NAMES)
@pytest.mark.parametrize("cid", ["tile-onoff-jitter", "tile-pointlight-ortho"])  # PIXEL, SAMPLE; four samples per pixel
def test_oracle_rays_across_the_crossing(oracle, cid, name):
    """The 16 pixels on either side of the crossing pixel: jitter from ``hostmodel.PCG(state, (seq + index) mod 2^64)``, the
    ray from ``tracer_fire_ray`` == the PT_HIT_RAY planes of the expected hit frame (tests/util.py: oracle_frame)."""
    case = vc.BY_ID[cid]
    p, cam = ss.params(case, name), vc.camera(case)
    assert p.n_ranks == 1 and p.samples_per_side == 2
    S, W, H, n = p.samples_per_side, p.width, p.height, ss.nsamp(p)
    assert {"tile-onoff-jitter": abi.PCG_PIXEL, "tile-pointlight-ortho": abi.PCG_SAMPLE}[cid] == p.pcg_mode
    oracle.set_sqr_mode(oracle.SQR_MUL)
    try:
        frame = util.oracle_frame(oracle, vc.scene(case), cam, p)
    finally:
        oracle.set_sqr_mode(oracle.SQR_POW)
    row, col = ss.crossing_pixel(case)
    at = row * W + col
    state, seq = ss.seeds(case, name)
    wrapped = 0
    for gpix in range(at - 16, at + 16):
        r, c = divmod(gpix, W)
        g = None
        for k in range(n):
            if p.pcg_mode == abi.PCG_SAMPLE:
                index = gpix * n + k
                g = hm.PCG(state, (seq + index) & M64)
            elif g is None:
                index = gpix
                g = hm.PCG(state, (seq + index) & M64)
            wrapped += seq + index >= ss.PAIRS[name][1]
            up = (k % S + g.random_float()) / S
            vp = (k // S + g.random_float()) / S
            ray = oracle.tracer_fire_ray(cam, W, H, c, r, up, vp)
            assert util.bits_equal(ray[0:3], frame.ray_origin[k, r, c]) and util.bits_equal(ray[3:6], frame.ray_dir[k, r, c]), (gpix, k)
    assert wrapped == 16 * n  # (the crossing pixel and the 15 behind it are at or beyond the boundary)


@pytest.mark.parametrize("name", ss.CROSSING_NAMES)
@pytest.mark.parametrize("cid", ["regions-hbm-deep", "path-one-lane",             # PIXEL, SAMPLE; one sample per pixel
                                 "sw-cull-0-path", "flagged-lean-lds-handover"])  # PIXEL, SAMPLE; four
def test_oracle_path_pixels_across_the_crossing(oracle, frames, cid, name):
    """Three pixels before and three at or after the crossing whose primary ray hits a shape that scatters (the path goes on:
    more than one ray per sample): two jitter draws and ONE ``radiance`` call per sample, from generators seeded with the sum
    taken in Python, == the oracle frame's pixel.  With one sample per pixel the pixel IS that call's value; with four it is
    their sum in sample order times 1 / 4 (imagetracer.py:83-101), which also holds ``pto_render`` to ``gpix * nsamp + k``."""
    case = vc.BY_ID[cid]
    p, cam, scene = ss.params(case, name), vc.camera(case), vc.scene(case)
    assert p.n_ranks == 1 and p.out_format == abi.OUT_F64 and p.samples_per_side in (1, 2)
    S, W, H, n = p.samples_per_side, p.width, p.height, ss.nsamp(p)
    image, _ = frames(case, None, *ss.seeds(case, name))
    state, seq = ss.seeds(case, name)
    row, col = ss.crossing_pixel(case)
    at = row * W + col

    def pixel(gpix):
        r, c = divmod(gpix, W)
        cum, rays, g = np.zeros(3), [], None
        for k in range(n):
            if p.pcg_mode == abi.PCG_SAMPLE or g is None:
                index = gpix * n + k if p.pcg_mode == abi.PCG_SAMPLE else gpix
                g = oracle.Pcg(state, (seq + index) & M64)
                h = hm.PCG(state, (seq + index) & M64)
                assert (g.state, g.inc) == (h.state, h.inc)
            up = (k % S + g.random_float()) / S
            vp = (k // S + g.random_float()) / S
            value, traced = oracle.radiance(scene, p, g, oracle.tracer_fire_ray(cam, W, H, c, r, up, vp))
            cum = cum + value
            rays.append(traced)
        return cum * (1 / S ** 2), min(rays), image[r, c]

    oracle.set_sqr_mode(oracle.SQR_MUL)
    try:
        for step, start in ((-1, at - 1), (1, at)):
            found, gpix = 0, start
            while found < 3:
                assert 0 <= gpix < W * H, f"{cid}: fewer than three scattering pixels on this side of the crossing"
                value, fewest, want = pixel(gpix)
                if fewest > 1:
                    assert util.bits_equal(value, want), (gpix, value, want)
                    found += 1
                gpix += step
    finally:
        oracle.set_sqr_mode(oracle.SQR_POW)


# ---- sensitivity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,name,mode", ss.SWEEP, ids=[ss.sweep_id(*s) for s in ss.SWEEP])
def test_frame_depends_on_the_whole_seed(frames, cid, name, mode):
    """The oracle's frame under the pair differs from the frames under (a) (45, 54), (b) the seeds reduced mod 2^32, (c) the
    sequence number plus 2^32 -- in a pixel BEFORE and in a pixel AFTER the crossing pixel (row-major), so that an error on
    either side of the boundary shows.  hi-state has no crossing: it differs anywhere.  So do the SEQ variants: SEQ is ONE stream
    entered at draw ``2 * nsamp * i``, no per-pixel sum is formed and nothing crosses a boundary inside the frame.

    x63: (b) is "seq + 1" instead.  Bit 63 of a sequence number is dropped by the generator's definition
    (``inc = (seq << 1) | 1`` mod 2^64), so reducing the pair's sequence number mod 2^63 is invisible by construction, and
    reducing it mod 2^32 as well tests nothing that x32 does not."""
    case = vc.BY_ID[cid]
    frame, _ = frames(case, mode, *ss.seeds(case, name, mode))
    W = frame.shape[1]
    flat = np.ascontiguousarray(frame).reshape(frame.shape[0] * W, -1)
    row, col = ss.crossing_pixel(case)
    at = vc.rows(case).index(row) * W + col
    for what, other_seeds in ss.contrast_seeds(case, name, mode):
        other, _ = frames(case, mode, *other_seeds)
        differs = (flat.view(np.uint8) != np.ascontiguousarray(other).reshape(flat.shape).view(np.uint8)).any(axis=1)
        if mode == abi.PCG_SEQ or ss.PAIRS[name][1] is None:
            assert differs.any(), f"{cid} {name}: the frame under {what} is the same"
        else:
            assert differs[:at].any(), f"{cid} {name}: no pixel before the crossing differs from the frame under {what}"
            assert differs[at + 1:].any(), f"{cid} {name}: no pixel after the crossing differs from the frame under {what}"


# ---- the catalogue's real-work conditions under the swept seeds -----------------------------------------------------------------
class _CachedOracle:
    """The oracle with the frames rendered above."""

    def __init__(self, oracle, frames, case):
        self.frames, self.case = frames, case
        self.SQR_MUL, self.SQR_POW, self.set_sqr_mode = oracle.SQR_MUL, oracle.SQR_POW, oracle.set_sqr_mode

    def render(self, scene, cam, par, sqr_mode):
        assert sqr_mode == self.SQR_MUL and par.pcg_mode != abi.PCG_SEQ
        return self.frames(self.case, None, par.path_state, par.path_seq)


@pytest.mark.parametrize("cid,name", [(c, n) for c in ss.PATH for n in ss.SEED_NAMES], ids=lambda v: v)
def test_swept_case_does_real_work_on_the_oracle(oracle, frames, monkeypatch, cid, name):
    """tests/test_variant_catalog.py::test_case_does_real_work_on_the_oracle itself -- the plan, the ``q_min_flagged`` side,
    the hand-over's ray budget -- with the catalogue handing out the swept params: which kernel the device lets work, and
    whether it hands pixels over, depends on what the seeds make the pixels do."""
    case = vc.BY_ID[cid]
    swept = ss.params(case, name)
    monkeypatch.setattr(vc, "params", lambda c: abi.copy_params(swept) if c.id == cid else pytest.fail(c.id))
    _real_work(_CachedOracle(oracle, frames, case), cid)
