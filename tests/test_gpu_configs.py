"""Every BASELINE.json configuration at its own size, through the C ABI with the options a caller gets by default
(C1 is the committed golden `c1_64_512*` in test_gpu_parity.py):

  C2  LANL-like          1024x1024 DVR
  C3  landing-gear-like  2048x2048 DVR (2 channels) + one implicit iso-surface
  C4  exajet-like, full  2048x2048 DVR                      (the bench line's workload)
  C5  exajet-like, full  4096x4096 DVR + iso-surface + AO, frames 0..15 accumulated

For each: (a) the oracle under the tolerance of tests/common.py — on the WHOLE frame for C2, C3 and C4 (every pixel
of the 1024^2 / 2048^2 frame; 16 host threads render them in about 2 / 20 / 30 s), on a 256x256 crop where the rays are
dense and on one across the silhouette for C5 (16 accumulated 4096^2 frames); (b) properties that need no oracle at full size: the kd walk and the LBVH restart pick
the same segments (bit-equal frames with the library powf), space skipping is image-neutral (KAT-7), launch order,
launch-order feedback and the wide march never change a pixel (also as rank 0 of 8, where the wide march engages)."""
import numpy as np
import pytest

from common import (ACCUM_ATOL, ACCUM_RTOL, AO_FLIP_BOUND, FLIP_BOUND, FLIP_FRACTION, MAX_ULP_SHIPPED, ULP_P999_SHIPPED, Case,
                    error_profile_line, po, ulp_profile)
from owlexabrick_amd import harness, scenes

pytestmark = pytest.mark.gpu

CROP = 96


def _windows(acc, W, H, CROP=CROP):
    """a fully covered CROP x CROP window nearest the image centre, and the one whose coverage is closest to one half
    (the silhouette), both on a 32-pixel grid; deterministic functions of the rendered frame"""
    cov = (acc[..., :3].sum(axis=-1) > 0).astype(np.float64)
    ii = np.zeros((H + 1, W + 1))
    ii[1:, 1:] = cov.cumsum(0).cumsum(1)
    best_dense, best_sil = None, None
    for y0 in range(0, H - CROP + 1, 32):
        for x0 in range(0, W - CROP + 1, 32):
            f = (ii[y0 + CROP, x0 + CROP] - ii[y0, x0 + CROP] - ii[y0 + CROP, x0] + ii[y0, x0]) / (CROP * CROP)
            dc = (x0 + CROP / 2 - W / 2) ** 2 + (y0 + CROP / 2 - H / 2) ** 2
            if f == 1.0 and (best_dense is None or dc < best_dense[0]):
                best_dense = (dc, x0, y0)
            key = (abs(f - 0.5), dc)
            if 0.2 < f < 0.8 and (best_sil is None or key < best_sil[0]):
                best_sil = (key, x0, y0)
    assert best_dense is not None and best_sil is not None, "frame has no dense / silhouette window"
    return {"dense": (best_dense[1], best_dense[2], best_dense[1] + CROP, best_dense[2] + CROP),
            "silhouette": (best_sil[1], best_sil[2], best_sil[1] + CROP, best_sil[2] + CROP)}


# Flip counts observed on the MI355X (profiles/parity_error_profile.txt): pixels beyond the per-pixel tolerance of
# tests/common.py (frames x 2e-5 + 1e-4 |accum|) — termination flips, and AO flips in the C5 windows; for form 1 against form 0
# the pixels beyond that tolerance ("moved") and beyond FORM_ACCUM_BOUND ("flips").  Each count is asserted to stay within
# 2 x observed + 5, next to the fraction bounds.
OBSERVED_FLIPS = {
    "C2": 0, "C3": 17, "C4": 18,
    "C2 form 1 vs form 0 moved": 54, "C2 form 1 vs form 0 flips": 6,
    "C3 form 1 vs form 0 moved": 306, "C3 form 1 vs form 0 flips": 17,
    "C4 form 1 vs form 0 moved": 327, "C4 form 1 vs form 0 flips": 7,
    "C2 form 1 vs oracle form 0 moved": 54, "C2 form 1 vs oracle form 0 flips": 6,
    "C3 form 1 vs oracle form 0 moved": 324, "C3 form 1 vs oracle form 0 flips": 22,
    "C4 form 1 vs oracle form 0 moved": 344, "C4 form 1 vs oracle form 0 flips": 12,
    "C2 form 0 vs oracle form 0": 0, "C3 form 0 vs oracle form 0": 16, "C4 form 0 vs oracle form 0": 18,
    "C4 x1.25": 2, "C4 three channels": 3,
    "C5 dense": 24, "C5 silhouette": 0, "C5 frame 0 centre": 41,
}
OBSERVED_PIXELS = {"C5 dense": 256 * 256 * 16, "C5 silhouette": 256 * 256 * 16, "C5 frame 0 centre": 1024 * 1024}
# An AO ray that flips hit / miss (cosf / sinf differ by ulps between libm and OCML) moves its frame's sample by half the
# surface colour (tests/common.py: AO_FLIP_BOUND).  Allowed per pixel and frame: twice the larger rate of the C5 windows above
# (41 of 1 048 576 in frame 0's centre window: 3.9e-5; the dense window has 24 of 65 536 x 16) = 7.8e-5.
AO_FLIP_FRACTION = 2 * max(OBSERVED_FLIPS[k] / OBSERVED_PIXELS[k] for k in OBSERVED_PIXELS)


def _within_observed(key, count):
    """a count of the table above: at most twice what was observed, plus 5"""
    return count <= 2 * OBSERVED_FLIPS[key] + 5


def _check_crop(acc_gpu, acc_cpu, win, frames, ao, what, key=None):
    x0, y0, x1, y1 = win
    g, o = acc_gpu[y0:y1, x0:x1].astype(np.float64), acc_cpu[y0:y1, x0:x1].astype(np.float64)
    d = np.abs(g - o)
    tol = frames * ACCUM_ATOL + ACCUM_RTOL * np.abs(o)
    flip_px = (d > tol).any(axis=-1)
    bad = int(flip_px.sum())
    n = d.shape[0] * d.shape[1]
    prof = ulp_profile(acc_cpu[y0:y1, x0:x1], acc_gpu[y0:y1, x0:x1], flip_px)
    print(f"{what}: {bad} of {n} pixels beyond {frames} x 2e-5 + 1e-4 |accum|, max |d accum| {d.max():.3g}")
    print(error_profile_line(dict(prof, what=what, flip_pixels=bad)))
    assert o[..., :3].sum() > 0, what
    if key is not None:
        assert _within_observed(key, bad), (what, key, bad, OBSERVED_FLIPS[key])
    # the shipped defaults (fast_math 1) on every pixel that is not a flip
    assert prof["max_ulp"] <= MAX_ULP_SHIPPED and prof["ulp_p999"] <= ULP_P999_SHIPPED, (what, prof)
    if ao:
        assert bad <= max(5, int(AO_FLIP_FRACTION * n * frames)), (what, bad, float(d.max()))
        assert d.max() <= frames * (AO_FLIP_BOUND + FLIP_BOUND), (what, float(d.max()))
        return
    # termination flips only (tests/common.py): rare, and bounded by the transmittance left at 0.98
    assert bad <= max(5, int(FLIP_FRACTION * n * frames)), (what, bad, float(d.max()))
    assert d.max() <= FLIP_BOUND * frames, (what, float(d.max()))


class Config:
    """one scene, one oracle scene, one renderer — built once per configuration"""

    def __init__(self, name, size, iso=None, ao=0, scale=1.0, fields=None):
        self.sc = scenes.config(name, scale=scale, fields=fields)
        nf = len(self.sc.fields)
        self.case = Case(self.sc, W=size, H=size, grad=1, iso=iso, ao=ao, xf_domains=[(0.0, 1.0)] * nf)
        self.R = self.case.hip_renderer()
        self.S = None

    def oracle(self):
        if self.S is None:
            self.S = self.case.oracle_scene()
        return self.S

    def render_frames(self, frames=1):
        rgba = None
        for f in range(frames):
            self.R.updateFrameID(f)
            rgba = self.R.render()
        return rgba, self.R.readAccum()

    def oracle_frames(self, win, frames=1, nthreads=16, basis_form=None):
        S, acc = self.oracle(), None
        if basis_form is not None:
            S.set_basis_form(basis_form)
        for f in range(frames):
            fs, P = self.case.oracle_state(S, frameID=f)
            _, acc, st = S.render(fs, P, self.case.W, self.case.H, window=win, accum=acc, nthreads=nthreads)
        if basis_form is not None:
            S.set_basis_form(self.case.basis_form)
        return acc

    def close(self):
        self.R.close()
        self.S = None


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def _properties(cfg, frames=1, lbvh=True):
    R = cfg.R
    R.updateFrameID(0)
    base = cfg.render_frames(frames)
    # ---- kd walk == LBVH restart, library powf (identical segments, samples and arithmetic) ----
    if lbvh:
        R.setOption("fast_math", 0)
        kd0 = cfg.render_frames(1)
        R.setOption("accel", 0)
        lb0 = cfg.render_frames(1)
        R.setOption("accel", 1)
        R.setOption("fast_math", 1)
        assert _same(kd0, lb0)
    # ---- the stack walk and the rope walk of the kd path find the same segments: bit-equal frames ----
    for walk in (1, 2):
        R.setOption("walk", walk)
        assert _same(cfg.render_frames(frames), base), f"walk {walk}"
    R.setOption("walk", 0)
    # ---- launch order / feedback / wide march never change a pixel ----
    for order in (0, 5):
        R.setOption("tile_order", order)
        assert _same(cfg.render_frames(frames), base), f"tile_order {order}"
    R.setOption("tile_order", 4)
    R.setOption("tile_feedback", 0)
    R.setOption("wide_march", 0)
    assert _same(cfg.render_frames(frames), base), "static order, one lane per ray"
    # as rank 0 of an 8-GPU job the feedback marks the critical tiles and the wide march takes them
    R.setShard(0, 8)
    static = cfg.render_frames(frames)
    R.setOption("tile_feedback", 1)
    R.setOption("wide_march", 1)
    for _ in range(3):                                   # measure, re-order + assign, steady state
        assert _same(cfg.render_frames(frames), static), "shard 0/8 with feedback + wide march"
    R.setShard(0, 1)
    # ---- KAT-7 at full size: space skipping is image-neutral ----
    with_skip = cfg.render_frames(1)
    R.setSpaceSkipping(False)
    no_skip = cfg.render_frames(1)
    R.setSpaceSkipping(True)
    assert np.abs(with_skip[1] - no_skip[1]).max() < 1e-5
    return base


def _oracle_crops(cfg, base_acc, frames=1, ao=0, what="", crop=CROP):
    wins = _windows(base_acc, cfg.case.W, cfg.case.H, crop)
    for k, win in wins.items():
        acc = cfg.oracle_frames(win, frames)
        _check_crop(base_acc, acc, win, frames, ao, f"{what} {k} {win}", key=f"{what} {k}")
    return wins


def _oracle_whole_frame(cfg, base_acc, what):
    """every pixel of the frame against the oracle (same tolerance as the crops: termination flips only)"""
    import time
    W, H = cfg.case.W, cfg.case.H
    t = time.time()
    acc = cfg.oracle_frames((0, 0, W, H))
    print(f"{what}: oracle rendered the whole {W}x{H} frame in {time.time() - t:.1f}s")
    _check_crop(base_acc, acc, (0, 0, W, H), 1, 0, f"{what} whole frame", key=what)
    d = np.abs(base_acc.astype(np.float64) - acc.astype(np.float64)).max(axis=-1)
    print(f"{what}: max |d accum| {d.max():.3g}, pixels beyond 2e-5 + 1e-4 |accum|: "
          f"{int((np.abs(base_acc.astype(np.float64) - acc) > ACCUM_ATOL + ACCUM_RTOL * np.abs(acc)).any(axis=-1).sum())} of {W * H}")


# Form 1 (the shipped default: basis sums per axis with fused multiply-adds) against form 0 (the reference's source order),
# stated in DESIGN.md 2: |d accum| <= 1e-3 (except for rays whose termination moves by one sample: <= 0.021, at most 0.02 % of
# the pixels), RGBA8 <= 1 LSB, at most 1 % of the pixels beyond the CPU-vs-GPU tolerance.  Each form is tied to the oracle in the same form bit-tightly elsewhere; this is the one comparison that tells
# what the default changes in the picture, on the whole frame at BASELINE size.
FORM_ACCUM_BOUND = 1e-3
FORM_PIXEL_FRACTION = 0.01


def _form1_vs_form0(cfg, what, oracle_form0=False, key=None):
    from owlexabrick_amd import harness as hs
    R = cfg.R
    R.setOption("basis_form", 1)
    rgba1, acc1 = cfg.render_frames(1)
    R.setOption("basis_form", 0)
    rgba0, acc0 = cfg.render_frames(1)
    R.setOption("basis_form", cfg.case.basis_form)
    d = np.abs(acc1.astype(np.float64) - acc0.astype(np.float64))
    moved = int((d > ACCUM_ATOL + ACCUM_RTOL * np.abs(acc0)).any(axis=-1).sum())
    lsb = int(np.abs(hs.unpack_rgba8(rgba1).astype(np.int32) - hs.unpack_rgba8(rgba0).astype(np.int32)).max())
    n = acc0.shape[0] * acc0.shape[1]
    flips = int((d > FORM_ACCUM_BOUND).any(axis=-1).sum())
    print(f"{what}: GPU form 1 vs GPU form 0, whole frame: max |d accum| {d.max():.3g}, {moved} of {n} pixels ({100.0 * moved / n:.3f} %) "
          f"beyond 2e-5 + 1e-4 |accum|, {flips} beyond 1e-3 (a ray that ends one sample earlier or later), RGBA8 max {lsb} LSB")
    # the association moves a pixel by at most 1e-3 — unless it moves the 0.98 termination decision of its ray by one sample,
    # which is worth up to 0.021 and allowed for the same fraction of pixels as between CPU and GPU (tests/common.py)
    assert lsb <= 1 and moved <= FORM_PIXEL_FRACTION * n, (what, lsb, moved)
    assert flips <= max(5, int(FLIP_FRACTION * n)) and d.max() <= FORM_ACCUM_BOUND + FLIP_BOUND, (what, flips, float(d.max()))
    key = key or what
    assert _within_observed(f"{key} form 1 vs form 0 moved", moved) and _within_observed(f"{key} form 1 vs form 0 flips", flips), \
        (what, moved, flips)
    if oracle_form0:
        # ... and the default GPU frame against the form-0 ORACLE itself (the definition), same bounds
        import time
        t = time.time()
        W, H = cfg.case.W, cfg.case.H
        o0 = cfg.oracle_frames((0, 0, W, H), basis_form=0).astype(np.float64)
        do = np.abs(acc1.astype(np.float64) - o0)
        moved_o = int((do > ACCUM_ATOL + ACCUM_RTOL * np.abs(o0)).any(axis=-1).sum())
        flips_o = int((do > FORM_ACCUM_BOUND).any(axis=-1).sum())
        print(f"{what}: GPU form 1 (default) vs ORACLE form 0 (source order), whole frame: max |d accum| {do.max():.3g}, {moved_o} of {n} "
              f"pixels ({100.0 * moved_o / n:.3f} %) beyond 2e-5 + 1e-4 |accum|, {flips_o} beyond 1e-3 (oracle {time.time() - t:.1f}s)")
        # a termination flip (<= 0.021) may sit on top of the association's own difference
        assert do.max() <= FORM_ACCUM_BOUND + FLIP_BOUND and moved_o <= FORM_PIXEL_FRACTION * n, (what, float(do.max()), moved_o)
        assert flips_o <= max(5, int(FLIP_FRACTION * n)), what
        assert _within_observed(f"{key} form 1 vs oracle form 0 moved", moved_o), (what, moved_o)
        assert _within_observed(f"{key} form 1 vs oracle form 0 flips", flips_o), (what, flips_o)
        # GPU form 0 against the form-0 oracle: the tight tolerance (termination flips only)
        _check_crop(acc0, o0.astype(np.float32), (0, 0, W, H), 1, 0, f"{what} GPU form 0 vs oracle form 0, whole frame",
                    key=f"{key} form 0 vs oracle form 0")


def test_c2_lanl_1024_dvr():
    cfg = Config("c2_lanl", 1024)
    try:
        base = _properties(cfg)
        _oracle_whole_frame(cfg, base[1], "C2")
        _form1_vs_form0(cfg, "C2", oracle_form0=True)
    finally:
        cfg.close()


def test_c3_gear_2048_dvr_two_channels_plus_iso():
    cfg = Config("c3_gear", 2048, iso=[(0.5, 0)])
    try:
        assert cfg.R.params.numPrimaryChannels == 2
        base = _properties(cfg)
        _oracle_whole_frame(cfg, base[1], "C3")
        _form1_vs_form0(cfg, "C3 (DVR of two channels + iso-surface)", oracle_form0=True, key="C3")
    finally:
        cfg.close()


@pytest.fixture(scope="module")
def exajet_full():
    """the bench scene (c4_exajet at scale 1.0: 6.4e8 cells), shared by C4 and C5"""
    box = {}

    def get(size, iso=None, ao=0):
        if "cfg" not in box:
            box["cfg"] = Config("c4_exajet", size, iso=iso, ao=ao)
        cfg = box["cfg"]
        if cfg.case.W != size or cfg.case.iso != iso or cfg.case.ao != ao:
            S = cfg.S
            case = Case(cfg.sc, W=size, H=size, grad=1, iso=iso, ao=ao, xf_domains=[(0.0, 1.0)])
            R = cfg.R
            lo, hi = R.voxelSpaceBounds
            cam = case.cam(lo, hi)
            R.resizeFrameBuffer((size, size))
            R.updateCamera(cam["pos"], cam["dir00"], cam["dirDu"], cam["dirDv"])
            iso_v, iso_c, iso_e = [0.0, 0.0], [0, 0], [0, 0]
            for i, spec in enumerate(iso or []):
                iso_v[i], iso_c[i], iso_e[i] = spec[0], spec[1], 1
            R.updateIsoValues(iso_v, iso_c, iso_e)
            R.frameState.ao.enabled, R.frameState.ao.length = int(case.ao), float(case.ao_length)
            cfg.case, cfg.S = case, S
        return cfg
    yield get
    if "cfg" in box:
        box["cfg"].close()


def test_c4_exajet_full_2048_dvr(exajet_full):
    cfg = exajet_full(2048)
    assert cfg.sc.num_cells > 6e8
    base = _properties(cfg)
    _oracle_whole_frame(cfg, base[1], "C4")
    _form1_vs_form0(cfg, "C4", oracle_form0=True)


def test_c5_exajet_full_4096_dvr_iso_ao_16_frames(exajet_full):
    cfg = exajet_full(4096, iso=[(0.5, 0)], ao=1)
    # property checks on 2 accumulated frames (surfaces pre-pass + march, SURF variants of the kernels) ...
    _properties(cfg, frames=2)
    # ... and the 16-frame accumulation ("16 spp") against the oracle on both crops
    cfg.R.setOption("tile_feedback", 1)
    cfg.R.setOption("wide_march", 1)
    base = cfg.render_frames(16)
    _oracle_crops(cfg, base[1], frames=16, ao=1, what="C5", crop=256)      # two 256 x 256 windows x 16 accumulated frames
    # ... and the 1024 x 1024 centre window of frame 0 (a sixteenth of the 4096^2 frame; ~15 s of oracle time)
    first = cfg.render_frames(1)
    win = (1536, 1536, 2560, 2560)
    _check_crop(first[1], cfg.oracle_frames(win, 1), win, 1, 1, "C5 frame 0, 1024^2 centre window", key="C5 frame 0 centre")
    # the iso-surface is really marched (the DVR in front of it leaves little of it visible with the default TF)
    cfg.R.updateFrameID(0)
    _, st = cfg.R.renderStats()
    assert st["iso_segments"] > 1e6 and st["iso_evals"] > 1e7 and st["samples"] > 1e9
    cfg.R.updateIsoValues([0, 0], [0, 0], [0, 0])
    plain = cfg.render_frames(1)
    cfg.R.updateIsoValues([0.5, 0], [0, 0], [1, 0])
    one = cfg.render_frames(1)
    assert np.abs(plain[1] - one[1]).max() > 5e-3


def test_field_beyond_4_gib_takes_the_64_bit_offsets():
    """maximum sizes: one scalar field larger than 4 GiB (exajet-like at scale 1.25: 1.2e9 cells, 4.8 GB per field).
    32-bit byte offsets and the wave-uniform-base loads are not valid here (exa_module: addr32 = 0), so the shipped
    march runs its general form with 64-bit addresses on real > 4 GiB offsets.  Same properties as the other
    configurations, and the WHOLE 512x512 frame against the oracle (every visible brick, wherever its cells lie)"""
    size = 512
    cfg = Config("c4_exajet", size, scale=1.25)
    try:
        assert cfg.sc.num_cells * 4 > 2 ** 32 and cfg.sc.num_cells < 2 ** 31
        base = _properties(cfg)
        win = (0, 0, size, size)
        _check_crop(base[1], cfg.oracle_frames(win), win, 1, 0, "C4 x1.25, whole frame", key="C4 x1.25")
    finally:
        cfg.close()


def test_c4_three_channels_full_scale_interleaved_copy_beyond_4_gib():
    """SURVEY 8(d)'s second data point for configs[3]: three DVR channels on the full exajet-like scene.  The
    channel-interleaved copy of the three fields (7.7 GB) is larger than 4 GiB, so the interleaved march runs its general
    64-bit address form on real > 4 GiB offsets while each field-major array still takes 32-bit offsets: the frame must
    equal the field-by-field march bit for bit, and the whole frame the oracle within the stated tolerance"""
    size = 384
    cfg = Config("c4_exajet", size, fields=3)
    try:
        assert cfg.R.params.numPrimaryChannels == 3 and cfg.sc.num_cells * 3 * 4 > 2 ** 32
        base = cfg.render_frames(2)
        cfg.R.setOption("interleave", 0)
        assert _same(cfg.render_frames(2), base), "field-by-field march"
        cfg.R.setOption("interleave", 1)
        cfg.R.setOption("brick_order", 1)
        assert _same(cfg.render_frames(2), base), "cells re-laid along the Morton curve"
        win = (0, 0, size, size)
        _check_crop(base[1], cfg.oracle_frames(win, frames=2), win, 2, 0, "C4 with three channels, whole frame",
                    key="C4 three channels")
    finally:
        cfg.close()
